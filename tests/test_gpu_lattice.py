"""The image-side kernels -- sdirt_psfnet_mlp, sdirt_local_psf_render (fp32 and fp16), sdirt_psfnet_render: together
PSFNet.render -- against float64 on lattice inputs (tests/lattice_f64.py, whose docstring carries the exactness
arguments and whose conditions tests/test_lattice_cpu.py checks).  On the lattice every product and every partial sum
in any order is exact, so the float64 answer rounded once where the kernel rounds is the only correct result:
torch.equal, no tolerance.  The one derived bound is on sdirt_psfnet_render, whose normalised weights leave the
lattice.  The float64 references run in torch on the GPU, which shares nothing with the kernels."""
import copy
import ctypes as C
import functools

import pytest
import torch

import lattice_f64 as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- fused MLP ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net(cfg):
    net, weights, biases = L.lattice_mlp(*cfg)
    return copy.deepcopy(net).to(DEV), weights, biases


def _mirrored(x):
    xm = x.clone()
    xm[:, 0] = -xm[:, 0]
    return xm


def _mlp_reference(cfg, n):
    """x [n,3] on the GPU and the float64 network at (x, y, z) and (-x, y, z): [2, n, out]."""
    _, weights, biases = _net(cfg)
    x = L.mlp_points(cfg, n).to(DEV)
    ref, report = L.mlp_f64(weights, biases, torch.cat((x, _mirrored(x))))
    L.assert_mlp_exact(report)                                         # on these very points
    assert report[-1]["nonzero"] > 0
    return x, ref.reshape(2, n, cfg[3])


def _check_fused(cfg, n):
    net = _net(cfg)[0]
    x, ref = _mlp_reference(cfg, n)
    got = net.forward_fused(x).reshape(n, cfg[3])
    assert got.dtype == torch.float16
    assert torch.equal(got.double(), ref[0]), _mismatch(got.double(), ref[0])
    both = net.forward_fused(x, mirror=True).reshape(2, n, cfg[3])
    assert torch.equal(both.double(), ref), _mismatch(both.double().reshape(2 * n, -1), ref.reshape(2 * n, -1))


def _mismatch(got, ref):
    """Which rows and output features differ (first few), for the assertion message."""
    bad = (got != ref).nonzero()
    rows, cols = bad[:, 0].unique(), bad[:, 1].unique()
    return (f"{len(bad)} of {ref.numel()} differ; rows {rows[:8].tolist()} .. {rows[-1:].tolist()} ({len(rows)}), "
            f"features {cols[:8].tolist()} .. {cols[-1:].tolist()} ({len(cols)}), "
            f"largest difference {float((got - ref).abs().max()):.4g}")


def test_fused_mlp_production_network():
    """3 -> 128 -> 512 x 9 -> 441, 300 rows (three tiles, the last of 44 rows)."""
    _check_fused(L.NET_PRODUCTION, 300)


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_fused_mlp_three_layers(n):
    """n_layers 3 (3 -> 32 -> 512 -> 25): the last layer follows a non-512 layer, with an unprimed weight ring; row
    counts around one tile."""
    _check_fused(L.NET_3_LAYERS, n)


def test_fused_mlp_sixteen_layers():
    """n_layers 16, the kernel's limit; activations in the thousands: round-to-nearest-even decides a quarter of
    the outputs."""
    _check_fused(L.NET_16_LAYERS, 200)


@pytest.mark.parametrize("out", L.IDLE_WAVE_OUTS)
def test_fused_mlp_output_widths_where_a_wave_falls_idle(out):
    """out_features either side of 128 / 256 / 384: where `128 * wave >= of` flips, and with it the prefetch of the
    last layer's weights during the penultimate layer."""
    _check_fused(L.net_idle_wave(out), 129)


def test_fused_mlp_persistent_loop():
    """2 * 128 * CUs + 77 rows: every workgroup takes at least two tiles, one a third; with mirror the right half
    starts in the middle of a tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _check_fused(L.NET_PERSISTENT, 2 * 128 * cus + 77)


@pytest.mark.parametrize("cfg,n,mirror", [(L.NET_3_LAYERS, 1, False), (L.NET_PERSISTENT, 129, False),
                                          (L.NET_OUT_121, 77, True)])
def test_fused_mlp_writes_inside_its_output_only(cfg, n, mirror):
    """sdirt_psfnet_mlp through the C ABI into a 16-byte-aligned slice in the middle of a larger buffer: the tail
    copy (whole 16-byte vectors while `i0 + 8 <= total`, then single values) leaves both guard bands untouched."""
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    net = _net(cfg)[0]
    x, ref = _mlp_reference(cfg, n)
    sides, of = (2 if mirror else 1), cfg[3]
    assert (sides * n * of) % 8 != 0                                    # the copy ends inside a vector
    buf, widths = net._packed()
    guard, sentinel = 4096, -3.0                                        # outputs are >= 0
    whole = torch.full((guard + sides * n * of + guard,), sentinel, dtype=torch.float16, device=DEV)
    out = whole[guard:guard + sides * n * of]
    assert out.data_ptr() % 16 == 0
    _lib.check(_lib.lib().sdirt_psfnet_mlp(dptr(buf), widths, len(widths) - 1, dptr(x.contiguous()), n,
                                           1 if mirror else 0, C.c_void_p(out.data_ptr()), stream_ptr(x.device)))
    torch.cuda.synchronize()
    assert bool((whole[:guard] == sentinel).all()) and bool((whole[guard + sides * n * of:] == sentinel).all())
    want = ref[:sides].reshape(sides * n, of)
    assert torch.equal(out.reshape(sides * n, of).double(), want), _mismatch(out.reshape(sides * n, of).double(), want)


# ---- per-pixel render ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", L.RENDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_render_kernels_return_the_float64_sum_bit_for_bit(shape):
    """local_dp_psf_render (fp32) == render_f64, local_psf_render_fast (fp16 arithmetic) == render_f64 rounded once
    to fp16, on every dispatch path of sdirt_local_psf_render and the loops no small shape enters."""
    from sdirt_amd import local_dp_psf_render, local_psf_render_fast
    B, Cn, H, W, ks = shape
    img = L.lattice_image(sum(shape), B, Cn, H, W).to(DEV)
    psf = L.lattice_psf(sum(shape) + 1, B, H, W, ks).to(DEV)
    left, right = L.render_f64(img.double(), psf.double(), ks)
    ref = torch.cat((left, right), dim=1)
    assert float(ref.max()) * 2 ** 11 < L.EXACT and float(ref.min()) >= 0 and float(ref.max()) > 1
    full = local_dp_psf_render(img, psf, kernel_size=ks)
    assert full.dtype == torch.float32
    assert torch.equal(full.double(), ref), _mismatch(full.double().reshape(-1, W), ref.reshape(-1, W))
    half = torch.cat(local_psf_render_fast(img, psf, kernel_size=ks), dim=1)
    want = L.round_f16(ref)
    assert not torch.equal(want, ref)                                   # the fp16 rounding decides bits
    assert torch.equal(half.double(), want), _mismatch(half.double().reshape(-1, W), want.reshape(-1, W))


@pytest.mark.parametrize("shape", L.PSFNET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_psfnet_render_against_float64(shape):
    """sdirt_psfnet_render against psfnet_render_f64: the kernel's own fp16 weights (sum, reciprocal and weights are
    exact or correctly rounded, hence reproducible), fp16 products, float64 sum."""
    from sdirt_amd.render_psf import psfnet_render
    B, Cn, H, W, ks = shape
    raw_l, raw_r = L.lattice_raw(sum(shape), B, H, W, ks)
    # a few dead kernels per side, at the ends of the pixel range and inside it
    dead_l = [(0, 0, 0), (B - 1, H - 1, W - 1), (0, H // 2, W // 3)]
    dead_r = [(0, 0, 1), (B - 1, H - 1, W - 2), (0, H // 2, W // 3)]
    for b, y, x in dead_l:
        raw_l[b, y, x] = 0
    for b, y, x in dead_r:
        raw_r[b, y, x] = 0
    img = L.lattice_image(sum(shape) + 1, B, Cn, H, W, floor=8).to(DEV)
    rl, rr = psfnet_render(img, raw_l.to(DEV), raw_r.to(DEV), ks)
    left, right, mag_l, mag_r = L.psfnet_render_f64(img, raw_l, raw_r, ks)
    # The kernel adds the same fp16 products in fp32 and rounds the sum to fp16 once.  Every fp32 addition errs by at
    # most 2^-24 of its partial sum, itself at most sum|terms| (first order).  A product passes through at most D
    # additions: a lane adds max(ceil(ks^2 / 64), ks) products serially on the wave and tiled paths (at most 2 ks on a
    # direct path), six butterfly levels follow, two are slack: D = 2 ks + 8.  So the fp32 sum lies within
    # D 2^-24 sum|terms| of the float64 one, and its fp16 rounding within half an fp16 ulp more.  That admits only
    # the two fp16 neighbours of ref, and leaves the choice open only where ref lies within D 2^-24 sum|terms| of a
    # midpoint between them -- a few percent of the outputs at worst: at least 90 % must be fp16(ref) bit for bit.
    D = 2 * ks + 8
    for side, got, ref, mag, dead in (("L", rl, left, mag_l, dead_l), ("R", rr, right, mag_r, dead_r)):
        assert got.shape == (B, Cn, H, W) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        err = (got.double() - ref).abs()
        bound = L.half_ulp(ref) + D * 2.0 ** -24 * mag
        worst = int((err - bound).argmax())
        equal = float((got.double() == L.round_f16(ref)).double().mean())
        print(f"psfnet_render {shape} {side}: largest |out - ref| {float(err.max()):.3e}; closest to its bound "
              f"{float(err.reshape(-1)[worst]):.3e} of {float(bound.reshape(-1)[worst]):.3e}; bit-equal to fp16(ref) "
              f"{100 * equal:.2f} %")
        assert bool((err <= bound).all()), (side, float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))
        assert equal >= 0.9, (side, equal)
        for b, y, x in dead:
            assert float(got[b, :, y, x].abs().max()) == 0, (side, b, y, x)
        assert float(got.max()) > 0.3
