"""The layered render's backward into the dual-pixel parameters h, f, w, the parts that need no GPU, on
the synthetic landings of tests/test_render_layers_cpu.py (dead rays on NaN, +-inf, +-3e38; binary and fractional
coverage; up to 16 layers) with a synthetic x_tan per ray, for r on both sides of 0.5:

  1. the product's torch restatement (layer_dp_grads_float64) against the independent one (tests/render_dp_grad_f64.py);
  2. ... and against torch.autograd through layer_sums_float64 -> images_from_sums, the weight rows formed by
     sub_pixel_areas at the same x_tan: the image loss covers gden as well;
  3. gden_from_image_grad, worked by hand on a 1 x 2 image, and with the photometric option;
  4. every new argument error; the entry in the header, the binding and the library."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_lens
import render_dp_grad_f64 as RD
from splat_f64 import fragile_x, gate_states, sub_pixel_areas
from test_render_layers_cpu import H, W, record, synthetic

ENTRY = "sdirt_render_layers_dp_grad"
U = 2.0 ** -53
DPS = [(0.78, 1.44, 0.3, 0.3), (0.78, 1.44, 0.3, 0.5), (0.78, 1.44, 0.3, 0.7)]


def scene(L, Ht, Wt, S, seed, shared, frac, dp):
    """synthetic's scene, an x_tan per ray that crosses every gate of the model (|x_tan| up to 1.1; the rays within
    1e-9 of a jump of the derivative are moved off it: two float64 restatements may round a boundary differently), and
    the adjoints gnum, gden."""
    px, py, ra, w, alpha, tex, inv = synthetic(L, Ht, Wt, S, seed=seed, shared=shared)
    rng = np.random.default_rng(seed + 7)
    if frac:
        alpha = np.where(rng.uniform(size=alpha.shape) < 0.5, rng.uniform(size=alpha.shape), alpha).astype(np.float32)
    x_tan = rng.uniform(-1.1, 1.1, ra.shape).astype(np.float32)
    bad = fragile_x(torch.from_numpy(x_tan), *dp, band=1e-9).numpy()
    x_tan = np.where(bad, x_tan + np.float32(1e-3), x_tan).astype(np.float32)
    assert not fragile_x(torch.from_numpy(x_tan), *dp, band=1e-9).any()
    gnum = rng.standard_normal((2, 3, H, W))
    gden = rng.standard_normal((2, H, W))
    return px, py, ra, w, alpha, tex, inv, x_tan, gnum, gden


# ------------------------------------------------------------------------------------ 1. torch against the restatement
@pytest.mark.parametrize("dp", DPS, ids=["r0.3", "r0.5", "r0.7"])
@pytest.mark.parametrize("with_gden", [True, False], ids=["gden", "no-gden"])
@pytest.mark.parametrize("L, Ht, Wt, S, shared, frac", [(1, 2, 3, 8, False, False), (2, 5, 141, 5, True, True),
                                                         (3, 11, 280, 8, False, True), (5, 1, 7, 5, False, False),
                                                         (16, 5, 9, 8, True, True)])
def test_the_product_s_restatement_equals_the_independent_one(L, Ht, Wt, S, shared, frac, with_gden, dp):
    """Both are float64 sums of the same n per-ray terms, whose factors are formed in different orders (closed formulas
    here, autograd through sub_pixel_areas there): within 2 n 2^-53 sum|term|, n the ray count."""
    from sdirt_amd.render_rt import layer_dp_grads_float64
    px, py, ra, w, alpha, tex, inv, x_tan, gnum, gden = scene(L, Ht, Wt, S, 700 + 10 * L + S, shared, frac, dp)
    gd = gden if with_gden else None
    ref = RD.dp_grads_f64(px, py, ra, x_tan, alpha, tex, inv, gnum, gd, *dp)
    got, scale = layer_dp_grads_float64(record(px, py, ra, w), x_tan, alpha, tex, inv, gnum, gd, dp, return_abs=True)
    assert got.dtype == torch.float64 and got.shape == (3,)
    n = ra.size
    tol = 2 * n * U * ref["scale"]
    worst = float((np.abs(got.numpy() - ref["grad"]) / tol).max())
    print(f"L {L}, r {dp[3]}: grad {ref['grad']}, worst |torch - restatement| / bound {worst:.3f}, {ref['n']} rays with a term")
    assert (np.abs(got.numpy() - ref["grad"]) <= tol).all(), worst
    assert (np.abs(scale.numpy() - ref["scale"]) <= tol).all()
    assert (ref["grad"] != 0).all() and (ref["scale"] > 0).all() and ref["n"] > 0.7 * (ra != 0).sum()
    # every gate of the model open and closed on some live rays (gi cannot close at r = 0.5, where |x2| <= 0.5 = r)
    for name, (opened, closed) in gate_states(torch.from_numpy(x_tan)[ra != 0], *dp).items():
        assert opened.any() and (closed.any() or (name == "gi" and dp[3] == 0.5)), name
    if L > 1:
        assert (ref["read"][ra != 0] < L).any() and (ref["read"][ra != 0] == L).any()    # walks that stopped at T == 0, and not
    # an opaque stack (alpha=None) is alpha == 1 in every bit
    none = layer_dp_grads_float64(record(px, py, ra, w), x_tan, None, tex, inv, gnum, gd, dp)
    ones = layer_dp_grads_float64(record(px, py, ra, w), x_tan, np.ones_like(alpha), tex, inv, gnum, gd, dp)
    assert torch.equal(none, ones)
    opaque = RD.dp_grads_f64(px, py, ra, x_tan, None, tex, inv, gnum, gd, *dp)
    assert (np.abs(none.numpy() - opaque["grad"]) <= 2 * n * U * opaque["scale"]).all()


def test_a_layer_behind_an_opaque_texel_is_not_read_whatever_it_holds():
    """Both restatements follow the forward's walk: a non-finite texture behind a fully opaque first layer changes nothing."""
    from sdirt_amd.render_rt import layer_dp_grads_float64
    dp = DPS[1]
    px, py, ra, w, alpha, tex, inv, x_tan, gnum, gden = scene(3, 5, 9, 5, 801, False, True, dp)
    alpha[0] = 1.0
    want = RD.dp_grads_f64(px, py, ra, x_tan, alpha, tex, inv, gnum, gden, *dp)
    base = layer_dp_grads_float64(record(px, py, ra, w), x_tan, alpha, tex, inv, gnum, gden, dp)
    tex[1:] = np.nan
    ref = RD.dp_grads_f64(px, py, ra, x_tan, alpha, tex, inv, gnum, gden, *dp)
    got = layer_dp_grads_float64(record(px, py, ra, w), x_tan, alpha, tex, inv, gnum, gden, dp)
    assert np.isfinite(ref["grad"]).all() and (ref["grad"] == want["grad"]).all() and (ref["read"][ra != 0] == 1).all()
    assert torch.equal(got, base) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------ 2. torch against autograd
@pytest.mark.parametrize("dp", DPS, ids=["r0.3", "r0.5", "r0.7"])
@pytest.mark.parametrize("photometric", [False, True], ids=["num/den", "photometric"])
@pytest.mark.parametrize("L, Ht, Wt, S, shared", [(1, 2, 3, 8, False), (3, 5, 9, 5, True), (16, 2, 3, 8, False)])
def test_the_product_s_restatement_equals_autograd_through_the_sums_and_the_image(L, Ht, Wt, S, shared, photometric, dp):
    """h, f, w are float64 leaves; the weight rows sub_pixel_areas makes of them enter layer_sums_float64's landing
    record, which is fp32: autograd casts every ray's adjoint A_side to fp32 once on its way back (one rounding, 2^-24
    relative), and forms it in another order in float64.  Tolerance: (2^-24 + 64 n 2^-53) times the sum over the rays
    of ra (sum_k |gnum_k c_k| + |gden|) |dw|, side by side -- magnitudes taken before the cancellation between the
    colour terms and gden inside A."""
    from sdirt_amd.render_rt import (gden_from_image_grad, gnum_from_image_grad, images_from_sums, layer_dp_grads_float64,
                                     layer_sums_float64)
    px, py, ra, w, alpha, tex, inv, x_tan, _, _ = scene(L, Ht, Wt, S, 900 + L, shared, True, dp)
    G = torch.from_numpy(np.random.default_rng(L).standard_normal((2, 3, H, W)))
    leaves = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in dp[:3]]
    t = torch.from_numpy(x_tan).double()
    sl, sr = sub_pixel_areas(t, *leaves, dp[3])
    base = record(px, py, ra, w)
    land = torch.cat((base[:1].double(), sr[None], sl[None], base[3:].double()))             # (w_L, w_R) = (s_r, s_l)
    num, den, _ = layer_sums_float64(land, alpha, tex, inv)
    (G * images_from_sums(num, den.unsqueeze(1), S, photometric)).sum().backward()
    auto = torch.stack([v.grad for v in leaves])
    with torch.no_grad():
        numd, dend = num.detach(), den.detach()
        gnum = gnum_from_image_grad(G, dend, S, photometric)
        gden = gden_from_image_grad(G, numd, dend, photometric)
        assert (gden is None) == photometric
        got = layer_dp_grads_float64(land.detach().float(), x_tan, alpha, tex, inv, gnum, gden, dp)
        # the scale: the same adjoint with every factor's magnitude
        gabs = None if gden is None else (G * numd).abs().sum(1) / torch.where(dend > 0, dend * dend, torch.ones_like(dend))
        _, scale = layer_dp_grads_float64(land.detach().float(), x_tan, alpha, np.abs(tex), inv, gnum.abs(), gabs, dp,
                                          return_abs=True)
    n = ra.size
    tol = (2.0 ** -24 + 64 * n * U) * scale
    worst = float(((auto - got).abs() / tol).max())
    print(f"L {L}, r {dp[3]}, {'photometric' if photometric else 'num/den'}: grad {got.tolist()}, "
          f"worst |autograd - restatement| / tolerance {worst:.3f}")
    assert bool(((auto - got).abs() <= tol).all()), worst
    assert bool((got.abs() > 0).all())


# ------------------------------------------------------------------------------------ 3. the helper
def test_gden_from_image_grad_by_hand():
    from sdirt_amd.render_rt import gden_from_image_grad, images_from_sums
    # one view pair, two planes, a 1 x 2 image; den of the right pixel of view 1 is 0
    G = torch.tensor([[[[1.0, 2.0]], [[3.0, -1.0]]], [[[0.5, 4.0]], [[-2.0, 8.0]]]])       # [2, 2, 1, 2]
    num = torch.tensor([[[[2.0, 1.0]], [[4.0, 3.0]]], [[[1.0, 5.0]], [[3.0, 7.0]]]], dtype=torch.float64)
    den = torch.tensor([[[2.0, 4.0]], [[0.5, 0.0]]], dtype=torch.float64)                  # [2, 1, 2]
    out = gden_from_image_grad(G, num, den)
    # view 0: -(1*2 + 3*4)/4 = -3.5, -(2*1 - 1*3)/16 = 0.0625; view 1: -(0.5*1 - 2*3)/0.25 = 22, den 0 -> 0
    assert out.dtype == torch.float64 and out.shape == (2, 1, 2)
    assert out.tolist() == [[[-3.5, 0.0625]], [[22.0, 0.0]]]
    # it is the adjoint of images_from_sums in den
    d = den.clone().requires_grad_()
    (images_from_sums(num, d.unsqueeze(1)) * G.double()).sum().backward()
    assert torch.equal(d.grad, out)
    # dimensions between the view and the pixel are summed over: [V, B, C, H, W]
    G5, num5 = G.reshape(2, 2, 1, 1, 2), num.reshape(2, 2, 1, 1, 2)
    assert torch.equal(gden_from_image_grad(G5, num5, den), out)
    # photometric: the image is num / spp, den has no adjoint
    assert gden_from_image_grad(G, num, den, photometric=True) is None
    with pytest.raises(ValueError, match="G and num_total must be one"):
        gden_from_image_grad(G, num[:, :1], den)
    with pytest.raises(ValueError, match="G and num_total must be one"):
        gden_from_image_grad(G, num, den[:1])


# ------------------------------------------------------------------------------------ 4. errors, entry
def test_header_declares_the_entry_and_the_library_exports_it():
    import ctypes as C
    from sdirt_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, code)
    assert "#define SDIRT_ABI_VERSION 4" in txt and "DESIGN.md §7r" in txt
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    n_args = len(re.search(r"int\s+%s\s*\((.*?)\);" % ENTRY, code, re.S).group(1).split(","))
    assert restype is C.c_int and len(argtypes) == n_args == 27
    h = _lib.lib()
    assert hasattr(h, ENTRY) and _lib.ABI_VERSION == 4 and h.sdirt_abi_version() == 4
    assert h.sdirt_render_layers_dp_grad(None, None, 0, None, None, 0.0, None, None, 0.0, 1, 1, 1, None, 1, None, None,
                                         None, None, 0, 1, 1, 1, None, None, None, None, None) != 0
    assert b"null lens" in h.sdirt_last_error()


def test_the_new_arguments_are_refused_before_anything_touches_the_gpu():
    from sdirt_amd import _lib
    from sdirt_amd.render_rt import layer_dp_grad_batch, layer_dp_grads_float64
    lens = make_lens("rf50mm", "cpu")
    lens.prepare_sensor(sensor_res=(4, 6), sensor_size=(1.0, 1.5))
    K = len(lens.surfaces)
    img, alpha, zs = torch.zeros(2, 3, 4, 6), torch.ones(2, 4, 6), [-500.0, -1000.0]
    pts = (torch.zeros(2, 4, 6), torch.zeros(2, 4, 6))
    kw = dict(scales=[5.0, 10.0], spp=2, pupil_points=pts)
    hl = torch.tensor(0.78, requires_grad=True)
    dpt = (hl, 1.44, 0.3, 0.5)
    # dp_grad=True with dp=None
    with pytest.raises(ValueError, match="dp_grad=True with dp=None"):
        lens.render_layers(img, alpha, zs, dp_grad=True, **kw)
    with pytest.raises(ValueError, match="dp_grad=True with dp=None"):
        lens.render_plane(img, -500.0, scale=5.0, spp=2, pupil_points=pts, dp_grad=True)
    with pytest.raises(ValueError, match="dp_grad=True with dp=None"):
        lens.render_rgbd(img, torch.full((2, 1, 4, 6), -1000.0), spp=2, scales=[10.0], pupil_points=pts, dp_grad=True)
    # return_sums with a recorded gradient
    with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
        lens.render_layers(img, alpha, zs, dp=dpt, dp_grad=True, return_sums=True, **kw)
    with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
        lens.render_plane(img, -500.0, scale=5.0, spp=2, pupil_points=pts, dp=dpt, dp_grad=True, return_sums=True)
    # ... but not where nothing is recorded: the call gets as far as asking for the GPU
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img, alpha, zs, dp=dpt, return_sums=True, **kw)                   # no dp_grad
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img, alpha, zs, dp=(0.78, 1.44, 0.3, 0.5), dp_grad=True, return_sums=True, **kw)   # no tensor
    with torch.no_grad(), pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img, alpha, zs, dp=dpt, dp_grad=True, return_sums=True, **kw)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img, alpha, zs, dp=dpt, dp_grad=True, **kw)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_rgbd(img, torch.full((2, 1, 4, 6), -1000.0), spp=2, scales=[10.0], pupil_points=pts, dp=dpt, dp_grad=True)
    # layer_dp_grad_batch
    trips, gnum, gden = [1] * K, torch.zeros(2, 3, 4, 6, dtype=torch.float64), torch.zeros(2, 4, 6, dtype=torch.float64)
    dp, inv = (0.78, 1.44, 0.3, 0.5), [1.0, 2.0]
    with pytest.raises(ValueError, match="no sub-pixel model"):
        layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips, gnum, gden, None)
    with pytest.raises(ValueError, match="r must be > 0 and f must differ from h"):
        layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips, gnum, gden, (0.78, 1.44, 0.3, 0.0))
    with pytest.raises(ValueError, match="r must be > 0 and f must differ from h"):
        layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips, gnum, gden, (0.78, 0.78, 0.3, 0.5))
    with pytest.raises(ValueError, match="2 layers need 2 depths and 2 scales"):
        layer_dp_grad_batch(lens, alpha, img, zs, [1.0], *pts, trips, gnum, gden, dp)
    with pytest.raises(ValueError, match="strictly descending"):
        layer_dp_grad_batch(lens, alpha, img, zs[::-1], inv, *pts, trips, gnum, gden, dp)
    with pytest.raises(ValueError, match="pupil points must be"):
        layer_dp_grad_batch(lens, alpha, img, zs, inv, pts[0], pts[1][:1], trips, gnum, gden, dp)
    with pytest.raises(ValueError, match="trip counts for a lens of"):
        layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips[:-1], gnum, gden, dp)
    for bad in (gnum.float(), gnum[:, :2], gnum[:1], None):
        with pytest.raises(ValueError, match="gnum must be float64"):
            layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips, bad, gden, dp)
    for bad in (gden.float(), gden[:1], gnum):
        with pytest.raises(ValueError, match="gden must be float64"):
            layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips, gnum, bad, dp)
    with pytest.raises(ValueError, match="layers differ"):
        layer_dp_grad_batch(lens, None, img, zs, [1.0], *pts, trips, gnum, gden, dp)
    with pytest.raises(ValueError, match="float32"):
        layer_dp_grad_batch(lens, None, img.double(), zs, inv, *pts, trips, gnum, gden, dp)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_dp_grad_batch(lens, alpha, img, zs, inv, *pts, trips, gnum, gden, dp)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_dp_grad_batch(lens, None, img[0], zs[:1], [1.0], *pts, trips, gnum, None, dp, x_tan=True)
    # layer_dp_grads_float64
    land, xt = torch.zeros(3 + 2 * 2, 2, 4, 6), torch.zeros(2, 4, 6)
    with pytest.raises(ValueError, match="landing record of 7 rows"):
        layer_dp_grads_float64(land[:5], xt, alpha, img, inv, gnum, gden, dp)
    with pytest.raises(ValueError, match="alpha has 2 layers"):
        layer_dp_grads_float64(land[:5], xt, alpha, img[0], [1.0], gnum, gden, dp)
    with pytest.raises(ValueError, match="x_tan must be"):
        layer_dp_grads_float64(land, xt[:1], alpha, img, inv, gnum, gden, dp)
    with pytest.raises(ValueError, match="gnum must be"):
        layer_dp_grads_float64(land, xt, alpha, img, inv, gnum[:1], gden, dp)
    with pytest.raises(ValueError, match="gden must be"):
        layer_dp_grads_float64(land, xt, alpha, img, inv, gnum, gden[:1], dp)
