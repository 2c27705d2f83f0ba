"""Inputs on a binary lattice and float64 restatements for the depth-network kernels of sdirt_amd/csrc/sdirt_dfdp.hip
(cost volume and its adjoint, window average, batch norm + ReLU, trilinear upsampling, disparity regression, tone
curves).  Not a test file.  tests/test_dfdp_f64_cpu.py checks every condition named here on the reference alone;
tests/test_gpu_dfdp_f64.py holds the kernels against it.

Every restatement is index arithmetic in float64 (or, for the cost volume's forward, a copy in the tensor's own type)
and shares nothing with the kernels or with the torch op it stands for.  As in tests/lattice_f64.py: operands that are
small integer multiples of a power of two make every product and every partial sum, in ANY order, exact in fp32, so the
float64 value rounded once WHERE THE KERNEL ROUNDS is the only result a correct kernel can return -> torch.equal.

Cost volume (cost_volume_gather, cost_volume_adjoint_f64).  cost[b, c2, i, h, w] is x[b, c2, h, w] for c2 < C and
y[b, c2 - C, h, w - gap] otherwise, gap = i - D // 2, wherever BOTH w and w - gap lie in [0, W), else 0.  The forward
is a copy: bit patterns, NaN payloads and the sign of zero included.  Adjoint on lattice_grad (m/16, |m| <= 64): an
input element collects at most D <= 64 of them, sum|terms| <= 64 * 64 units of 2^-4 < 2^24: exact in fp32; the result is
that sum, kept in fp32 or rounded once to fp16.  fp16 holds every multiple of 2^-4 below 128, so the rounding decides
bits only when |sum| > 128: the `hot` gradients (m in 49..64) with D = 64 reach sums of 128 .. 256, where a kernel that
accumulated in fp16 would round at every step.

Window average (window_average_f64) on lattice_values(.., 128) (m/16, |m| <= 128: exact in fp16): a window of up to
32 x 32 sums to at most 2^10 * 2^7 = 2^17 units < 2^24: column sums, their four-way split and the LDS pass are exact in
any order.  The kernels return fp32(sum * fp32(1 / k^2)) rounded to T: for k a power of two the product is exact and the
result is the mean rounded once; for other k the fp16 result is a deliberate DOUBLE rounding (to fp32, then to fp16),
restated as such: the float64 product of an 18-bit sum and a 24-bit reciprocal is exact, .float() is the first
rounding, .to(T) the second.

Batch norm + ReLU (bn_lattice_tables, bn_relu_f64): x and mean multiples of 2^-4 within +-16, invstd in {1/4 .. 4},
gamma a multiple of 1/4 within +-4, beta a multiple of 2^-4 within +-16.  x - mean: a multiple of 2^-4 within +-32;
times gamma: of 2^-6 within +-128; times invstd (a power of two): of 2^-8 within +-512; plus beta: of 2^-8 within +-528
< 2^18 units: every step exact in fp32 in the kernel's order gamma * (x - mean) * invstd + beta.  The result is that
value, clamped (y < 0 -> +0, so -0.0 and NaN pass), rounded once to T.  Channel 0 has gamma = 0, beta = -0.0 (results
+0 and -0.0), channel 1 gamma = beta = 0; fp16 keeps 11 bits, so multiples of 2^-8 above 8 are rounded, many on ties.

Trilinear upsampling (trilinear_f64 with lerp_exact): out = 2 in - 1 (or 4 in - 3) with align_corners gives the scale
(in - 1) / (out - 1) = 1/2 (1/4) exactly in fp32, src = scale * dst exact, weights in {0, 1/2, 1} (multiples of 1/4).
On lattice_values(.., 128) every term is a multiple of 2^-4 * 4^-3 = 2^-10 below 8: sums exact in fp32; the result is
rounded once to T.  Any wrong corner index or i1 clamp is a bit difference.

Disparity regression (disparity_f64, peaked_cost): in-plane x 4 without align_corners has src = (dst + 1/2) / 4 - 1/2:
weights multiples of 1/8; depth 20 -> 20 is the identity, 10 -> 20 and 32 -> 64 have weights 1/4, 3/4.  On values m/16,
|m| <= 128 every interpolated v[i] is a multiple of 2^-4 * 8^-2 * 4^-1 = 2^-12 within +-8 and v[i] - max within +-16 <
2^17 units: exact in fp32.  The softmin gets exact arguments; only expf (kappa ulp), the sum (D - 1 additions), the
division, the product with the shift and the expectation (D - 1 additions) round.  With u = 2^-24 and e_i the exact
exponentials: |fl(e_i) / e_i - 1| <= 2 kappa u, the sum adds (D - 1) u, the quotient u, the product u, the expectation
(D - 1) u: |err| <= (4 kappa + 2 D + 2) u sum_i p_i |s_i| to first order (disparity_bound).  kappa: the ROCm
installation carries no HIP math documentation (no table of ulp errors for expf), so kappa = 2 is used.
peaked_cost gives every input pixel one winning plane (-8 against 4 .. 8) that changes slowly across the map, so that
the largest p_i exceeds 0.5 on most output pixels and the expectation depends on the planes, not on a uniform average.

Tone curves (tone_f64): both curves in float64 on the kernel's fp32 constants, with a running bound on what the fp32
op sequence can differ by: every operation propagates the bound of its operands rigorously (|1/(v+d) - 1/v| <=
e / (|v| (|v| - e)), |ab| products, 1-Lipschitz min / max) and adds one rounding u (|v| + e) + 2^-149 -- division and
reciprocal are correctly rounded under -fno-fast-math.  The bound is a function of the input alone.

Derived bounds where the lattice cannot reach (general values, non-dyadic ratios): the restatement takes the kernel's
fp32 INPUTS TO THE ARITHMETIC as given -- the interpolation weights computed in numpy float32 by the kernel's own rule
(lerp_f32; reproducible: the library is built with -ffp-contract=off), the fp32 tables of _bn_tables -- evaluates in
float64 and bounds the kernel by gamma_n = n u / (1 - n u) times sum|terms|, n its count of fp32 roundings on the
longest path (6 for the trilinear sum: product, sum, product, sum, product, sum; 4 for batch norm), plus half an ulp
of fp16 where the result is rounded to fp16.  The products of three 24-bit weights are not exact in float64; their
2^-53 is 2^-29 of u."""
import numpy as np
import torch

from lattice_f64 import EXACT, half_ulp, round_f16                  # noqa: F401  (re-exported for the tests)

U24 = 2.0 ** -24                                                    # fp32 unit roundoff
KAPPA_EXPF = 2                                                      # ulp bound assumed for expf (see above)


def gamma_n(n):
    return n * U24 / (1 - n * U24)


def lattice_values(seed, shape, m_hi, lo=None):
    """float64 tensor of m/16, m uniform in [lo, m_hi] (lo = -m_hi by default)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-m_hi if lo is None else lo, m_hi + 1, tuple(shape), generator=g).double() / 16


def lattice_grad(seed, shape, hot=False):
    """Gradients m/16 with |m| <= 64; hot: m in 49..64 (sums over 64 planes pass 128, where fp16 rounds)."""
    return lattice_values(seed, shape, 64, 49 if hot else None)


def to_type(x64, dtype):
    """float64 -> dtype through fp32: one rounding whenever x64 is exact in fp32 (every lattice result is)."""
    return x64.float().to(dtype)


# ---- cost volume ----------------------------------------------------------------------------------------------------
def _cv_index(D, W, device):
    gap = torch.arange(D, device=device) - D // 2                                    # [D]
    w = torch.arange(W, device=device)
    wy = w[None, :] - gap[:, None]                                                   # [D, W]: the column of y
    return wy, (wy >= 0) & (wy < W)                                                  # (w itself is always inside)


def cost_volume_gather(x, y, d_max):
    """x, y [B,C,H,W] of any dtype -> [B,2C,D,H,W] of that dtype, as a gather (a copy: bits preserved)."""
    B, C, H, W = x.shape
    wy, ok = _cv_index(d_max, W, x.device)
    left = x[:, :, None, :, :].expand(B, C, d_max, H, W)
    right = y[:, :, :, wy.clamp(0, W - 1)].permute(0, 1, 3, 2, 4)                    # [B,C,H,D,W] -> [B,C,D,H,W]
    both = torch.cat((left, right), 1)
    return torch.where(ok[None, None, :, None, :], both, torch.zeros((), dtype=x.dtype, device=x.device))


def cost_volume_adjoint_f64(g, d_max):
    """g [B,2C,D,H,W] float64 -> (gx, gy, terms): each input element's sum over the volume elements it was copied to;
    terms = the largest sum of |g| any element collects."""
    B, C2, D, H, W = g.shape
    C = C2 // 2
    assert D == d_max
    _, ok = _cv_index(D, W, g.device)                                                # ok[i, w]: volume column w holds data
    m = ok[None, None, :, None, :].double()
    gx = (g[:, :C] * m).sum(2)
    # y[.., w'] went to column w' + gap of plane i whenever that column exists
    gap = torch.arange(D, device=g.device) - D // 2
    wv = torch.arange(W, device=g.device)[None, :] + gap[:, None]                    # [D, W']
    inside = ((wv >= 0) & (wv < W))[None, None, :, None, :].double()
    idx = wv.clamp(0, W - 1)[None, None, :, None, :].expand(B, C, D, H, W)
    gy = (torch.gather(g[:, C:], 4, idx) * inside).sum(2)
    terms = max(float((g[:, :C].abs() * m).sum(2).max()), float((torch.gather(g[:, C:].abs(), 4, idx) * inside).sum(2).max()))
    return gx, gy, terms


# (B, C, H, W) per d_max: the narrowest accepted width d_max // 2 + 1 and the issue's widths, every channel count at the
# small widths (C 8 / 32: the 16-byte form in fp16 / fp32, 1 / 3: element-wise), two at the wide ones
CV_DMAX = (1, 2, 5, 7, 20)


def cv_cases(d_max):
    widths = sorted({d_max // 2 + 1} | {w for w in (3, 4, 5, 9, 33, 130) if w > d_max // 2})
    return [(2 if c < 8 else 1, c, 3, w) for w in widths for c in ((1, 3, 8, 32) if w <= 16 else (3, 8))]


CV_HOT = (1, 3, 2, 70, 64)                                           # (B, C, H, W, d_max) of the hot-gradient adjoint


def special_values(x):
    """x with NaN (two payloads), +-inf and -0.0 written into its first elements (in place on a flat view)."""
    f = x.view(-1)
    vals = [float("nan"), float("inf"), float("-inf"), -0.0]
    for j, v in enumerate(vals):
        f[(7 * j) % f.numel()] = v
    return x


# ---- window average -------------------------------------------------------------------------------------------------
def window_average_f64(x, k, dtype):
    """x [B,C,H,W] float64 on the lattice -> (result as the kernels round it, float64; sum|terms| in units of 2^-4)."""
    B, C, H, W = x.shape
    s = torch.zeros((B, C, H // k, W // k), dtype=torch.float64, device=x.device)
    a = torch.zeros_like(s)
    for i in range(k):
        for j in range(k):
            s += x[:, :, i::k, j::k]
            a += x[:, :, i::k, j::k].abs()
    inv = float(np.float32(1) / np.float32(k * k))
    return (s * inv).float().to(dtype).double(), float(a.max()) * 16


def wa_values(seed, shape):
    """m/16 with m in -16..128: mostly positive, so that window sums pass fp16's 11 bits and means reach 4 .. 8."""
    return lattice_values(seed, shape, 128, -16)


WA_K = (1, 3, 4, 6, 7, 8, 32)


def wa_planar_widths(k):
    """W in {k, the largest multiple below 256, the first multiple >= 256 (a second trip of the column loop whenever it
    exceeds 256), 257 k (OW = 257: a second trip of the output loop)}."""
    return sorted({k, k * (255 // k), k * -(-256 // k), k * -(-257 // k), 257 * k})


WA_NHWC_C = (8, 24, 40, 128, 1024, 2048)
WA_NHWC_K = (1, 2, 3, 8, 32)                                        # (3: s * fp32(1/9) is not s / 9 rounded once)


# ---- batch norm + ReLU ----------------------------------------------------------------------------------------------
def bn_lattice_tables(seed, C):
    """(mean, invstd, gamma, beta) float64 [C] on the lattice; channel 0: gamma 0, beta -0.0; channel 1: gamma 0, beta 0."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randint(-256, 257, (C,), generator=g).double() / 16
    invstd = 2.0 ** torch.randint(-2, 3, (C,), generator=g).double()
    gamma = torch.randint(-16, 17, (C,), generator=g).double() / 4
    beta = torch.randint(-256, 257, (C,), generator=g).double() / 16
    gamma[0], beta[0] = 0.0, -0.0
    if C > 1:
        gamma[1], beta[1] = 0.0, 0.0
    return mean, invstd, gamma, beta


def bn_relu_f64(x, tables, relu):
    """x float64 [outer, C, ...] -> (y, mag): gamma * (x - mean) * invstd + beta in the kernel's order (the order fixes
    the sign of a zero result), y < 0 -> +0 when relu; mag = |gamma (x - mean) invstd| + |beta|."""
    shape = [1, -1] + [1] * (x.dim() - 2)
    mean, invstd, gamma, beta = (t.to(x.device).double().view(shape) for t in tables)
    t = gamma * (x - mean) * invstd
    y = t + beta
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)
    return y, t.abs() + beta.abs()


BN_PIXEL_MAJOR_C = (3, 5, 32, 250, 256, 264, 2048)


# ---- linear interpolation -------------------------------------------------------------------------------------------
def lerp_exact(out, inp, align):
    """torch's source index from integer arithmetic -> (i0, i1, l0, l1, src): src = dst (in - 1) / (out - 1) with
    align_corners, max((dst + 1/2) in / out - 1/2, 0) without; l1 = frac(src), exact whenever it is dyadic."""
    dst = np.arange(out, dtype=np.int64)
    if align:
        num, den = (dst * (inp - 1), out - 1) if out > 1 else (0 * dst, 1)
    else:
        num, den = np.maximum((2 * dst + 1) * inp - out, 0), 2 * out
    i0 = num // den
    l1 = (num % den) / den
    return i0, np.minimum(i0 + 1, inp - 1), 1.0 - l1, l1, i0 + l1


def lerp_f32(out, inp, align):
    """The kernel's rule (lerp_scale / lerp_at of sdirt_dfdp.hip) in numpy float32, operation by operation."""
    f = np.float32
    dst = np.arange(out).astype(f)
    if align:
        scale = f(inp - 1) / f(out - 1) if out > 1 else f(0)
        src = scale * dst
    else:
        scale = f(inp) / f(out)
        src = np.maximum(scale * (dst + f(0.5)) - f(0.5), f(0))
    assert src.dtype == np.float32
    i0 = src.astype(np.int64)
    assert int(i0.max()) <= inp - 1 and int(i0.min()) >= 0           # what the kernel would read
    l1 = src - i0.astype(f)
    l0 = f(1) - l1
    assert l0.dtype == np.float32
    return i0, i0 + (i0 < inp - 1), l0.astype(np.float64), l1.astype(np.float64), src.astype(np.float64)


def trilinear_f64(x, size, align, rule=lerp_exact):
    """x [B,C,D0,H0,W0] float64 -> (out, mag) [B,C,*size]: the eight-corner weighted sum and the sum of |terms|."""
    ax = []
    for o, i in zip(size, x.shape[2:]):
        i0, i1, l0, l1, _ = rule(o, i, align)
        ax.append([(torch.as_tensor(i0, device=x.device), torch.as_tensor(l0, device=x.device)),
                   (torch.as_tensor(i1, device=x.device), torch.as_tensor(l1, device=x.device))])
    out = torch.zeros(x.shape[:2] + tuple(size), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    for di, ld in ax[0]:
        xd = x[:, :, di]
        for hi, lh in ax[1]:
            xh = xd[:, :, :, hi]
            for wi, lw in ax[2]:
                wgt = ld[:, None, None] * lh[None, :, None] * lw[None, None, :]
                v = xh[:, :, :, :, wi]
                out += wgt * v
                mag += wgt * v.abs()
    return out, mag


UP_IN = ((1, 2, 3), (2, 3, 5), (5, 1, 2), (3, 5, 1), (2, 2, 2))     # (D0, H0, W0), mixed
UP_C = (1, 5, 8, 64)


# ---- disparity regression -------------------------------------------------------------------------------------------
def peaked_cost(seed, B, D0, H0, W0):
    """[B,D0,H0,W0] float64 on the lattice: background m/16 with m in 64..128, one winning plane per pixel at -8; the
    winner is constant over 2 x 2 pixels and moves by one plane from block to block."""
    x = lattice_values(seed, (B, D0, H0, W0), 128, 64)
    b, h, w = torch.meshgrid(torch.arange(B), torch.arange(H0), torch.arange(W0), indexing="ij")
    win = (seed + b + h // 2 + w // 2) % D0
    x.scatter_(1, win[:, None], -8.0)
    return x


def disparity_f64(cost, maxdisp, hw, rule=lerp_exact):
    """cost [B,D0,H0,W0] float64 -> dict: disp [B,1,H,W] (trilinear without align_corners to [maxdisp, H, W], softmin
    over the planes, expectation over the shifts floor(-maxdisp / 2) + i), pmax (largest probability per pixel),
    S = sum p |s|, M = largest sum|w x| of a pixel's planes, R = largest |v_i - max v|."""
    vol, mag = trilinear_f64(cost[:, None], (maxdisp,) + tuple(hw), False, rule)
    v = -vol[:, 0]
    d = v - v.max(1, keepdim=True)[0]
    e = torch.exp(d)
    p = e / e.sum(1, keepdim=True)
    first = (-maxdisp) // 2                                            # Python's floor division: -3 for 5
    s = torch.arange(first, first + maxdisp, device=cost.device).double().view(1, -1, 1, 1)
    return dict(disp=(p * s).sum(1, keepdim=True), pmax=p.max(1)[0], S=(p * s.abs()).sum(1, keepdim=True),
                M=mag[:, 0].max(1, keepdim=True)[0], R=d.abs().max(1, keepdim=True)[0], v=v)


def disparity_bound(r, D, exact_arguments):
    """Bound on |kernel - r['disp']| per pixel.  Exact softmin arguments (the lattice at dyadic ratios): the text
    above.  Otherwise every argument v_i - max carries the error of two interpolated values (6 roundings each on
    sum|w x| <= M) and of the subtraction: a = 2 gamma_6 M + u R; exp turns it into a relative error exp(a) - 1 of e_i,
    hence at most exp(2 a) - 1 of p_i.  2^-100 covers exponentials that underflow in fp32."""
    b = (4 * KAPPA_EXPF + 2 * D + 2) * U24 * r["S"] + 2.0 ** -100
    if not exact_arguments:
        a = 2 * gamma_n(6) * r["M"] + U24 * r["R"]
        b = b + torch.expm1(2 * a) * r["S"]
    return b


# (d_in, maxdisp, H0, W0): the three instantiations, the kernel's limits, odd maxdisp, border clamps
DISP_DYADIC = ((20, 20, 5, 6), (10, 20, 5, 6), (32, 64, 2, 5), (20, 20, 1, 1), (10, 20, 1, 2), (20, 20, 2, 1),
               (5, 5, 5, 2), (7, 7, 2, 2), (16, 32, 1, 5))
DISP_GENERAL = ((3, 5, 5, 7), (7, 13, 2, 5), (1, 4, 2, 3), (10, 20, 5, 6), (20, 20, 2, 5))


# ---- tone curves ----------------------------------------------------------------------------------------------------
TONE_DECIMAL = ((0.89129432, 0.27217316, -0.00246187), (5.94018909e-01, 1.20060450e+01, -5.24983855e-03))
TONE_F32 = tuple(tuple(float(np.float32(c)) for c in row) for row in TONE_DECIMAL)


class _Run:
    """A float64 value and a rigorous bound on the distance of the fp32 evaluation from it."""

    def __init__(self, v, e=None, rounded=True):
        self.v = v
        e = torch.zeros_like(v) if e is None else e
        self.e = e + U24 * (v.abs() + e) + 2.0 ** -149 if rounded else e

    def mulc(self, c):
        return _Run(self.v * c, self.e * abs(c))

    def addc(self, c):
        return _Run(self.v + c, self.e)

    def recip(self):
        return _Run(1 / self.v, self.e / (self.v.abs() * (self.v.abs() - self.e).clamp(min=1e-300)))

    def mul(self, o):
        return _Run(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def add(self, o):
        return _Run(self.v + o.v, self.e + o.e)

    def rsub1(self):
        return _Run(1 - self.v, self.e)

    def clampc(self, lo=None, hi=None):
        return _Run(self.v.clamp(min=lo, max=hi), self.e, rounded=False)


def _f32c(num, den):
    return float(np.float32(num) / np.float32(den))


def tone_f64(x, mode, consts=TONE_F32, f32_constants=True, blend=False):
    """mode 0: degamma(img) = fit_degamma(255 img); mode 1: clip(fit_gamma(l) / 255, 0, 1) -> (value, bound), float64.
    f32_constants: the reciprocals 1/100, 1/255, 1/a and 1e-9 as the fp32 numbers the kernel multiplies by / adds."""
    (a1, b1, c1), (a2, b2, c2) = consts
    r100, r255 = (_f32c(1, 100), _f32c(1, 255)) if f32_constants else (1 / 100, 1 / 255)
    ra1, ra2 = (_f32c(1, a1), _f32c(1, a2)) if f32_constants else (1 / a1, 1 / a2)
    eps = float(np.float32(1e-9)) if f32_constants else 1e-9
    x = _Run(x.double(), rounded=False)
    if mode == 0:
        x = x.mulc(255.0)
        lo = x.mulc(a1).addc(b1).recip().addc(c1).recip()
        hi = x.mulc(a2).addc(b2).recip().addc(c2).recip()
        t = x.mulc(r100).clampc(hi=1.0)
        out = hi.mul(t).add(lo.mul(t.rsub1()))
    else:
        r = x.addc(eps).recip()
        x1 = r.addc(-c1).recip().addc(-b1).mulc(ra1)
        x2 = r.addc(-c2).recip().addc(-b2).mulc(ra2)
        t = x1.add(x2).mulc(0.5).mulc(r100)
        if blend:                                                     # the unclamped blend weight (tone_inputs' knee)
            return t.v, t.e
        t = t.clampc(hi=1.0)
        out = x2.mul(t).add(x1.mul(t.rsub1())).mulc(r255).clampc(lo=0.0, hi=1.0)
    return out.v, out.e


TONE_LUM_MAX = 1200.0
TONE_N = 256 * 256 * 16 + 77                                        # one partial second pass of k_tone's loop


def tone_inputs(mode, n=TONE_N):
    """fp32 [n]: a dense ramp with 0, 1, the knee of the blend (code value 100) and its fp32 neighbours on both sides
    written over the first elements.  mode 0: images in [0, 1].  mode 1: luminances in [0, TONE_LUM_MAX], a little past
    degamma(1) = 1155 so that both clips act; the knee is where the blend weight of fit_gamma passes 1."""
    x = torch.linspace(0, 1 if mode == 0 else TONE_LUM_MAX, n, dtype=torch.float64).float()
    knee = np.float32(100.0 / 255.0)
    if mode == 1:
        lo, hi = 0.0, TONE_LUM_MAX                                    # bisection on the blend weight passing 1
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            t = tone_f64(torch.tensor([mid], dtype=torch.float64), 1, blend=True)[0]
            lo, hi = (mid, hi) if float(t) < 1.0 else (lo, mid)
        knee = np.float32(lo)
    around = [knee]
    for _ in range(4):
        around = [np.nextafter(around[0], np.float32(0))] + around + [np.nextafter(around[-1], np.float32(1e9))]
    head = [0.0, 1.0] + [float(a) for a in around]
    x[:len(head)] = torch.tensor(head, dtype=torch.float32)
    return x


# ---- launch caps (the grid-stride loops) ------------------------------------------------------------------------------
CAP_64 = 256 * 64 * 256                                             # threads of a launch capped at 256 * 64 blocks
CAP_16_BLOCKS = 256 * 16                                            # blocks of sdirt_tone_curve / pixel-major sdirt_bn_relu


def partial_second_pass(total, cap):
    return cap < total < 2 * cap
