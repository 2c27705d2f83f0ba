"""Inputs on a binary lattice and float64 restatements for the image-side kernels (sdirt_psfnet_mlp,
sdirt_local_psf_render, sdirt_psfnet_render), for tests that ask for bit equality.  Not a test file.

The idea, three times: give a kernel operands that are small integer multiples of a power of two.  Every product is
then exact in the kernel's number format and every partial sum, in ANY order, is exact in fp32 -- so the float64
answer, rounded once where the kernel rounds, is the only result a correct kernel can return, whatever its tiling,
lane mapping or reduction tree.  tests/test_lattice_cpu.py checks the conditions below on the reference alone;
tests/test_gpu_lattice.py holds the kernels against it with torch.equal.

Fused MLP (lattice_mlp, lattice_points, mlp_f64), lattice unit u = 2^-5:
  * inputs, biases and (inductively) activations are integer multiples of u; weights are small integers, so every
    term of a layer's sum is an integer multiple of u.  Rounding such a number to fp16 keeps it a multiple of u (fp16
    holds every multiple of u up to 2^11 u = 64; beyond that its spacing is a power of two times u);
  * a sum of multiples of u, in any order and any grouping, is exact in fp32 while  sum|terms| + |bias| < 2^24 u:
    every partial sum is then a multiple of u below 2^24 u, which fp32 holds (mlp_f64 reports that quantity per layer);
  * the one fp16 rounding of that exact sum (round to nearest even) is a function of the sum alone, and max(., 0)
    commutes with it.
  Sparse +-1 rows after the first layer keep the activations far below fp16's 65504 however deep the network.

Per-pixel render (lattice_image, lattice_psf, render_f64 of tests/render_f64.py): image values k/32 with k < 32,
kernel values m/64 with m < 64, dense.
  * a product is k m 2^-11 with k m < 2^11: exact in fp16 (and in fp32), at least 2^-11 when nonzero: never subnormal;
  * a sum of up to 65^2 such products stays below 65^2 * 31 * 63 < 2^24 units of 2^-11: exact in fp32 in any order;
  * so the fp32 kernel must return render_f64 exactly and the fp16 kernel render_f64 rounded once to fp16.

Fused pred + render (lattice_raw, psfnet_render_f64): the normalised weights leave the lattice, so there the test
carries a derived bound; what the lattice still gives: the kernel's sum of raw values is exact in fp32, hence its
fp16 rounding, the reciprocal and every fp16 weight are the kernel's bit for bit (both kernels divide correctly
rounded), no weight and no product with a nonzero image value of lattice_image(..., floor=8) is an fp16 subnormal."""
import functools

import torch
import torch.nn.functional as F

from render_f64 import render_f64                                    # noqa: F401  (re-exported for the tests)

U = 2.0 ** -5                                                       # the MLP's lattice unit
EXACT = 2.0 ** 24                                                   # fp32 holds every integer below it


# ---- fused MLP ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_mlp(seed, h4, hidden_layers, out, nnz_hi):
    """psfnet_arch.MLP 3 -> h4 -> 512 -> (512 -> 512) x hidden_layers -> out with lattice parameters
    -> (net, weights, biases): the module (CPU, fp32) and its parameters as float64 lists.
    Layer 0: dense integers in [-2, 2].  Every later layer: per output row k ~ U{1..nnz_hi} nonzeros at random
    columns, each +-1.  Biases: integers in [-4, 8] times u."""
    from sdirt_amd.psfnet_arch import MLP
    g = torch.Generator().manual_seed(seed)
    net = MLP(3, out, hidden_features=512, hidden_layers=hidden_layers)
    net.net[0] = torch.nn.Linear(3, h4)
    net.net[2] = torch.nn.Linear(h4, 512)
    weights, biases = [], []
    with torch.no_grad():
        for l, m in enumerate(net._linears()):
            rows, cols = m.weight.shape
            if l == 0:
                w = torch.randint(-2, 3, (rows, cols), generator=g).double()
            else:
                k = torch.randint(1, nnz_hi + 1, (rows, 1), generator=g)
                rank = torch.rand(rows, cols, generator=g).argsort(1).argsort(1)     # a random permutation per row
                sign = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
                w = sign * (rank < k)
            b = torch.randint(-4, 9, (rows,), generator=g).double() * U
            m.weight.copy_(w)
            m.bias.copy_(b)
            weights.append(w)
            biases.append(b)
    return net, weights, biases


def lattice_points(seed, n):
    """[n, 3] fp32: x, y in {-32..32} u, z in {0..32} u -- the network's input range, exact in fp16."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(-32, 33, (n, 2), generator=g)
    z = torch.randint(0, 33, (n, 1), generator=g)
    return (torch.cat((xy, z), 1).double() * U).float()


def mlp_f64(weights, biases, x):
    """Per layer h = fp16(relu(h @ W.T + b)) in float64 on x's device -> (out [n, out] float64, report).
    report[l] = dict(terms: largest sum|terms| + |bias| in units of u (exactness needs < 2^24), amax: largest
    activation after rounding (fp16 overflows at 65504), nonzero: share of nonzero activations, rounded: share of
    activations the fp16 rounding changed).  The sums are exact in float64 and, under the condition on `terms`, in
    fp32: the float64 -> fp32 -> fp16 conversion below rounds once."""
    h = x.double()
    report = []
    for w, b in zip(weights, biases):
        w, b = w.to(h.device), b.to(h.device)
        terms = h.abs() @ w.abs().T + b.abs()
        s = torch.relu(h @ w.T + b)
        h = s.float().half().double()
        report.append(dict(terms=float(terms.max()) / U, amax=float(h.max()), nonzero=float((h != 0).double().mean()),
                           rounded=float((h != s).double().mean())))
    return h, report


def assert_mlp_exact(report):
    """The conditions of the exactness argument, on mlp_f64's report."""
    for l, r in enumerate(report):
        assert r["terms"] < EXACT, (l, r)
        assert r["amax"] < 65504, (l, r)


# ---- per-pixel render ---------------------------------------------------------------------------------------------
def lattice_image(seed, B, C, H, W, floor=0):
    """[B,C,H,W] fp32, values k/32 with k in 0..31; values below floor/32 are 0."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 32, (B, C, H, W), generator=g)
    return (k * (k >= floor)).float() / 32


def lattice_psf(seed, B, H, W, ks):
    """[B,H,W,2,ks,ks] fp32, values m/64 with m in 0..63, dense."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 64, (B, H, W, 2, ks, ks), generator=g).float() / 64


def render_f16_products_f64(img, psf, ks):
    """The _fast renderer's arithmetic restated: image and kernels rounded to fp16, every product rounded to fp16,
    the products summed in float64 -> (left, right, abs_left, abs_right), unrounded float64 [B,C,H,W]; abs_* is the
    sum of the products' magnitudes."""
    b, c, h, w = img.shape
    pad = (ks - 1) // 2
    P = F.pad(img.float(), (pad, pad, pad, pad), mode="replicate").half().float()
    K = psf.reshape(b, h, w, 2, ks, ks).half().float().permute(3, 0, 1, 2, 4, 5).unsqueeze(2)    # [2,B,1,H,W,ks,ks]
    out = torch.zeros((2, b, c, h, w), dtype=torch.float64, device=img.device)
    mag = torch.zeros_like(out)
    for i in range(ks):
        for j in range(ks):
            # fp16 x fp16 is exact in fp32 (22 significant bits): .half() is the product's single rounding
            t = (K[..., i, j] * P[:, :, ks - 1 - i:ks - 1 - i + h, ks - 1 - j:ks - 1 - j + w]).half().double()
            out += t
            mag += t.abs()
    return out[0], out[1], mag[0], mag[1]


def round_f16(x):
    """float64 -> nearest fp16 value, as float64.  Through fp32, which is exact for the sums of this module (integer
    multiples of 2^-24 below 2^24 units), so this rounds once."""
    return x.float().half().double()


# ---- fused pred + render ------------------------------------------------------------------------------------------
def raw_m_hi(ks):
    """Largest numerator m of lattice_raw: with values in [128, m_hi] / 1024 a kernel's sum is at most
    ks^2 m_hi / 1024 <= 448, so a normalised weight is at least (1/8) / 448 (1 - 2^-10) > 2^-12 and its product with
    an image value >= 1/4 at least 2^-14, fp16's smallest normal number; m < 2^11 keeps the value exact in fp16."""
    return min(2047, 448 * 1024 // (ks * ks))


def lattice_raw(seed, B, H, W, ks):
    """Network outputs (raw_l, raw_r), each [B,H,W,ks,ks] fp16: a quarter of the taps 0, the others m/1024 with
    m in 128..raw_m_hi(ks).  A kernel's sum is below 2^24 units of 2^-10: exact in fp32 in any order."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(128, raw_m_hi(ks) + 1, (2, B, H, W, ks, ks), generator=g)
    m = m * (torch.randint(0, 4, m.shape, generator=g) > 0)
    raw = (m.double() / 1024).half()
    return raw[0], raw[1]


def psfnet_weights(raw_l, raw_r, ks):
    """PSFNet.pred on raw outputs as sdirt_psfnet_render defines it -> fp16 [B,H,W,2,ks,ks] on the CPU:
    stack(left, fliplr(right)); tot = fp16(sum raw); inv = fp32(1 / fp32(tot + 1e-9f)); w = fp16(fp32(raw) * inv).
    The sum is taken in float64 (exact, as the kernel's fp32 sum is on lattice_raw); the rest in fp32 / fp16 torch
    ops on the CPU, whose division is IEEE.  A zero-sum kernel gets weights 0 * 1e9 = 0."""
    raw = torch.stack((raw_l.cpu(), torch.flip(raw_r.cpu(), dims=[-1])), dim=-3)                 # [...,2,ks,ks]
    tot = raw.double().sum((-1, -2), keepdim=True).float().half()
    inv = 1.0 / (tot.float() + torch.tensor(1e-9, dtype=torch.float32))
    return (raw.float() * inv).half()


def psfnet_render_f64(img, raw_l, raw_r, ks):
    """psfnet.py:317-336 + the _fast renderer: psfnet_weights, then render_f16_products_f64 on img's device
    -> (left, right, abs_left, abs_right), unrounded float64; the kernel returns left / right rounded to fp16."""
    b, _, h, w = img.shape
    wts = psfnet_weights(raw_l.reshape(b, h, w, ks, ks), raw_r.reshape(b, h, w, ks, ks), ks)
    return render_f16_products_f64(img, wts.to(img.device), ks)


def half_ulp(x):
    """Half an fp16 ulp at |x|: 2^(floor(log2|x|) - 11), at least 2^-25 (half the subnormal spacing)."""
    _, e = torch.frexp(x.double().abs())                             # |x| = m 2^e, m in [0.5, 1): floor(log2|x|) = e - 1
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 12).clamp(min=2.0 ** -25).where(
        x != 0, torch.full_like(x, 2.0 ** -25, dtype=torch.float64))


# ---- the cases of tests/test_gpu_lattice.py, shared with tests/test_lattice_cpu.py ----------------------------------
# (seed, h4, hidden_layers, out, nnz_hi): lattice_mlp's arguments.  The activations grow by about sqrt(mean k / 2)
# per sparse layer (k nonzeros per row, half of the inputs alive): nnz_hi is chosen per depth so that the deep layers
# exceed 64 -- where fp16 no longer holds every multiple of u, so that the rounding (to nearest even) decides bits --
# and stay far below 65504.  Measured on these seeds (tests/test_lattice_cpu.py asserts the conditions): production
# net, largest activation 1.2e4, 38 % of the outputs changed by the rounding; 16 layers, 4.7e3 and 26 %; the shallow
# nets stay near 100, where only a few values are rounded.
NET_PRODUCTION = (1, 128, 8, 441, 16)
NET_3_LAYERS = (2, 32, 0, 25, 8)
NET_16_LAYERS = (3, 64, 13, 512, 8)
NET_PERSISTENT = (4, 128, 1, 441, 16)
IDLE_WAVE_OUTS = (1, 127, 128, 129, 256, 257, 384, 385)


def net_idle_wave(out):
    # one seed per width: a seed whose single output feature is dead under the ReLU would test nothing at out = 1
    return (50 + out, 96, 1, out, 16)


NET_OUT_121 = net_idle_wave(121)                                    # the mirrored case of the output-bounds test
MLP_NETS = (NET_PRODUCTION, NET_3_LAYERS, NET_16_LAYERS, NET_PERSISTENT, NET_OUT_121) + tuple(
    net_idle_wave(o) for o in IDLE_WAVE_OUTS)


def mlp_points(cfg, n):
    """The points of the case (network cfg, n rows)."""
    return lattice_points(1000 * cfg[0] + n % 1000, n)


# (B, C, H, W, ks) of sdirt_local_psf_render: the dispatch shapes of test_render_kernels_equal_a_plain_torch_convolution
# in tests/test_gpu_next_rows.py, then
RENDER_SHAPES = [(2, 3, 9, 13, 21), (1, 3, 5, 8, 21), (1, 3, 33, 70, 21), (1, 3, 4, 97, 21), (1, 1, 7, 10, 21),
                 (1, 3, 6, 11, 7), (1, 4, 5, 9, 33), (1, 3, 5, 9, 49), (1, 1, 4, 7, 65),
                 # one, two and three 64-pixel chunks of the wave kernel, odd tails of its two-pixel pipeline,
                 (2, 3, 3, 64, 21), (1, 3, 3, 65, 21), (1, 3, 2, 130, 21),
                 # B H > 4096 / groups: a workgroup of the row-mapped kernel walks several pixel groups (3 groups of 8
                 # pixels on 2 workgroups per row); a run starts at float 2 ks^2 (row W + x0), so its LDS misalignment
                 # sh is 0 throughout at W 20, ks 5 and alternates 0 / 2 from row to row at W 17, ks 7,
                 (1, 1, 3000, 20, 5), (1, 4, 2100, 17, 7),
                 # the direct kernel with 4 channels
                 (1, 4, 3, 9, 65)]
# ... and of sdirt_psfnet_render: the wave kernel (ks 21, C 3; three chunks / a batch of rows), the tiled kernel with
# 16 pixels per tile (ks 21 C 1, ks 5, ks 9) and with 8 (ks 31; 35 pixels: a last tile of 3), and more than
# 16 * 16384 tiles' worth of pixels: a second trip of the tiled kernel's grid-stride loop
PSFNET_SHAPES = [(1, 3, 5, 130, 21), (2, 3, 40, 56, 21), (1, 1, 9, 13, 21), (2, 1, 9, 13, 5), (1, 4, 7, 33, 9),
                 (1, 3, 5, 7, 31), (1, 1, 290, 905, 3)]
