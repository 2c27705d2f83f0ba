"""The layered render's backward, the parts that need no GPU, on the synthetic landings of
tests/test_render_layers_cpu.py (dead rays on NaN, +-inf, +-3e38; binary and fractional coverage; up to 16 layers):

  1. exact differences: sum gnum num of §7p's numpy forward is affine in one texel of alpha and linear in one of tex,
     so its value with the texel at 1 minus its value with the texel at 0 IS the gradient -- every texel of the small
     textures, against the numpy restatement of §7q (tests/render_layers_grad_f64.py) and the product's torch one;
  2. the product's torch restatement (layer_grads_float64) against the numpy one within §7q's bound;
  3. ... and against torch.autograd through layer_sums_float64 on float32 leaves;
  4. the gnum helper; every new argument error; the entry in the header, the binding and the library."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_lens
import render_layers_f64 as RL
import render_layers_grad_f64 as RG
from test_render_layers_cpu import H, W, record, synthetic

ENTRY = "sdirt_render_layers_grad"
U = 2.0 ** -53


def scene(L, Ht, Wt, S, seed, shared, frac):
    px, py, ra, w, alpha, tex, inv = synthetic(L, Ht, Wt, S, seed=seed, shared=shared)
    rng = np.random.default_rng(seed + 1)
    if frac:                                   # fractional coverage on half of the texels, 0 / 1 on the others
        alpha = np.where(rng.uniform(size=alpha.shape) < 0.5, rng.uniform(size=alpha.shape), alpha).astype(np.float32)
    gnum = rng.standard_normal((2, 3, H, W))
    return px, py, ra, w, alpha, tex, inv, gnum


def dot_forward(px, py, ra, w, alpha, tex, inv, gnum):
    num = RL.layer_sums_f64(px, py, ra, w, alpha, tex, inv)[0]
    return float((gnum * num).sum())


# ------------------------------------------------------------------------------------ 1. exact differences
@pytest.mark.parametrize("frac", [False, True], ids=["binary", "fractional"])
@pytest.mark.parametrize("L, Ht, Wt, S, shared", [(1, 2, 3, 8, False), (3, 2, 3, 5, False), (3, 2, 3, 8, True),
                                                   (5, 1, 1, 5, False), (16, 1, 2, 8, True)])
def test_the_restated_gradient_is_the_forward_s_exact_difference_in_every_texel(L, Ht, Wt, S, shared, frac):
    """F(texel = 1) - F(texel = 0) for F = sum gnum num.  Tolerance, per texel: both F carry the forward restatement's
    rounding -- every elementary product |gnum| wr T a w_j |tex| passes at most 7 (lookup) + 3 L (g, T, c) + 3 (wr, the
    term) + S (the sum over s) + 1 (gnum num) roundings, and numpy's pairwise sum of the V T H W products log2 of that
    many more -- so |error of F| <= 2 (3 L + S + 11 + log2 P) 2^-53 Fabs with Fabs the same forward on |gnum| and |tex|
    (all its terms are non-negative); to that the gradient restatement's own §7q bound is added."""
    from sdirt_amd.render_rt import layer_grads_float64
    px, py, ra, w, alpha, tex, inv, gnum = scene(L, Ht, Wt, S, 300 + 10 * L + S, shared, frac)
    ref = RG.layer_grads_f64(px, py, ra, w, alpha, tex, inv, gnum)
    own_a, own_t = (t.numpy() for t in layer_grads_float64(record(px, py, ra, w), alpha, tex, inv, gnum))   # the product's
    P = gnum.size
    eps_f = 2 * (3 * L + S + 11 + np.log2(P)) * U
    worst = 0.0

    def check(arr, pos, got, bound):
        nonlocal worst
        keep = arr[pos]
        F = []
        for v in (1.0, 0.0):
            arr[pos] = v
            F.append((dot_forward(px, py, ra, w, alpha, tex, inv, gnum),
                      dot_forward(px, py, ra, w, alpha, np.abs(tex), inv, np.abs(gnum))))
        arr[pos] = keep
        tol = eps_f * (F[0][1] + F[1][1]) + bound
        for g in got:
            err = abs((F[0][0] - F[1][0]) - g)
            worst = max(worst, err / max(tol, 1e-300))
            assert err <= tol, (pos, err, tol)

    for pos in np.ndindex(alpha.shape):
        check(alpha, pos, (ref["galpha"][pos], own_a[pos]), RG.bound(ref["n_alpha"][pos], L, ref["abs_alpha"][pos]))
    for pos in np.ndindex(tex.shape):
        check(tex, pos, (ref["gtex"][pos], own_t[pos]), RG.bound(ref["n_tex"][pos], L, ref["abs_tex"][pos]))
    print(f"L {L}, {Ht} x {Wt}, {'shared' if shared else 'per-layer'}: worst |difference - gradient| / tolerance {worst:.3f}")
    assert np.abs(ref["galpha"]).max() > 0 and np.abs(ref["gtex"]).max() > 0
    if L > 1:
        # the case the forward never reads: a ray stopped by an opaque texel with coverage behind it
        stopped = (ref["T_before"][:-1] != 0) & (ref["a"][:-1] == 1) & (ref["a"][1:] != 0) & (ra != 0)
        assert stopped.any()


# ------------------------------------------------------------------------------------ 2. torch against numpy
@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("frac", [False, True], ids=["binary", "fractional"])
@pytest.mark.parametrize("shared", [False, True], ids=["per-layer", "shared"])
@pytest.mark.parametrize("L, Ht, Wt, S", [(1, 2, 3, 8), (2, 5, 141, 5), (3, 11, 280, 8), (5, 1, 7, 5), (16, 5, 9, 8),
                                          (2, 1, 1, 8), (3, 7, 1, 5)])
def test_the_product_s_gradient_restatement_equals_the_independent_one(L, Ht, Wt, S, shared, frac, views):
    from sdirt_amd.render_rt import layer_grads_float64
    px, py, ra, w, alpha, tex, inv, gnum = scene(L, Ht, Wt, S, 400 + 10 * L + Wt + S, shared, frac)
    gnum = gnum[:views]
    ref = RG.layer_grads_f64(px, py, ra, w[:views], alpha, tex, inv, gnum)
    got = layer_grads_float64(record(px, py, ra, w), torch.from_numpy(alpha), torch.from_numpy(tex), inv,
                              torch.from_numpy(gnum), views=views, return_abs=True)
    ga, gt, aa, at = (t.numpy() for t in got)
    assert ga.shape == alpha.shape and gt.shape == tex.shape and ga.dtype == gt.dtype == np.float64
    for arr in (ga, gt, aa, at):
        assert np.isfinite(arr).all()
    for name, g, ab in (("alpha", ga, aa), ("tex", gt, at)):
        bound = RG.bound(ref["n_" + name], L, ref["abs_" + name])
        worst = float((np.abs(g - ref["g" + name]) / np.maximum(bound, 1e-300)).max())
        print(f"g{name}: worst |torch - numpy| / bound {worst:.3f}")
        assert (np.abs(g - ref["g" + name]) <= bound).all(), worst
        assert (np.abs(ab - ref["abs_" + name]) <= bound).all()
        assert (np.abs(ref["g" + name]) <= ref["abs_" + name] * (1 + 1e-12)).all() and (ref["abs_" + name] > 0).any()
    # an opaque stack (alpha=None) is alpha == 1: the same colour gradient in every bit, no coverage gradient
    none_a, none_t = layer_grads_float64(record(px, py, ra, w), None, torch.from_numpy(tex), inv, torch.from_numpy(gnum),
                                         views=views)
    ones_a, ones_t = layer_grads_float64(record(px, py, ra, w), torch.ones(L, Ht, Wt), torch.from_numpy(tex), inv,
                                         torch.from_numpy(gnum), views=views)
    assert none_a is None and torch.equal(none_t, ones_t)
    opaque = RG.layer_grads_f64(px, py, ra, w[:views], None, tex, inv, gnum)
    assert opaque["galpha"] is None
    assert (np.abs(none_t.numpy() - opaque["gtex"]) <= RG.bound(opaque["n_tex"], L, opaque["abs_tex"])).all()


# ------------------------------------------------------------------------------------ 3. torch against autograd
@pytest.mark.parametrize("shared", [False, True], ids=["per-layer", "shared"])
@pytest.mark.parametrize("L, Ht, Wt, S", [(1, 2, 3, 8), (3, 5, 9, 5), (16, 2, 3, 8)])
def test_the_product_s_gradient_restatement_equals_autograd_through_the_sums(L, Ht, Wt, S, shared):
    """torch.autograd through layer_sums_float64 on float32 leaves: the float64 adjoints are cast to fp32 where they
    reach the leaf (a shared image once per layer, added in fp32), so the two agree within (L + 2) 2^-24 sum|term| plus
    §7q's bound."""
    from sdirt_amd.render_rt import layer_grads_float64, layer_sums_float64
    px, py, ra, w, alpha, tex, inv, gnum = scene(L, Ht, Wt, S, 500 + L, shared, True)
    land = record(px, py, ra, w)
    a = torch.from_numpy(alpha).requires_grad_()
    t = torch.from_numpy(tex).requires_grad_()
    num = layer_sums_float64(land, a, t, inv)[0]
    (torch.from_numpy(gnum) * num).sum().backward()
    assert a.grad.dtype == t.grad.dtype == torch.float32
    ga, gt, aa, at = layer_grads_float64(land, alpha, tex, inv, gnum, return_abs=True)
    n = 4 * S * H * W                                          # no texel has more terms than there are taps
    for name, auto, g, ab in (("alpha", a.grad, ga, aa), ("tex", t.grad, gt, at)):
        tol = (L + 2) * 2.0 ** -24 * ab + torch.from_numpy(RG.bound(n, L, ab.numpy()))
        worst = float(((auto.double() - g).abs() / tol.clamp_min(1e-300)).max())
        print(f"g{name}: worst |autograd - restatement| / tolerance {worst:.3f}")
        assert bool(((auto.double() - g).abs() <= tol).all()), worst
        assert float(g.abs().max()) > 0


# ------------------------------------------------------------------------------------ 4. helper, errors, entry
def test_gnum_from_image_grad():
    from sdirt_amd.render_rt import gnum_from_image_grad, images_from_sums
    g = torch.Generator().manual_seed(3)
    G = torch.randn(2, 3, 4, 5, generator=g)
    den = torch.rand(2, 4, 5, generator=g, dtype=torch.float64)
    den[0, 1, 2], den[1, 0, 0], den[1, 3, 4] = 0.0, 0.0, -1.0          # den <= 0: the image is 0 there, and so is gnum
    out = gnum_from_image_grad(G, den)
    assert out.dtype == torch.float64 and out.shape == G.shape
    want = torch.where(den.unsqueeze(1) > 0, G.double() / den.unsqueeze(1), torch.zeros((), dtype=torch.float64))
    assert torch.equal(out, want) and bool((out[0, :, 1, 2] == 0).all()) and bool((out[1, :, 3, 4] == 0).all())
    assert bool(torch.isfinite(out).all())
    # [V, B, C, H, W] (render_plane) broadcasts den over both dimensions between
    G5 = torch.randn(2, 2, 3, 4, 5, generator=g)
    assert torch.equal(gnum_from_image_grad(G5, den)[:, 1], gnum_from_image_grad(G5[:, 1], den))
    # it is the adjoint of images_from_sums: autograd through that function gives the same
    num = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64).requires_grad_()
    (images_from_sums(num, den.unsqueeze(1)) * G.double()).sum().backward()
    assert torch.allclose(num.grad, out, rtol=1e-15, atol=0)
    # photometric: G / spp everywhere, whatever den holds
    ph = gnum_from_image_grad(G, den, spp=8, photometric=True)
    assert torch.equal(ph, G.double() / 8.0)
    num.grad = None
    (images_from_sums(num, den.unsqueeze(1), 8, True) * G.double()).sum().backward()
    assert torch.equal(num.grad, ph)


def test_header_declares_the_entry_and_the_library_exports_it():
    import ctypes as C
    from sdirt_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, code)
    assert "#define SDIRT_ABI_VERSION 4" in txt and "DESIGN.md §7q" in txt
    assert "ADDED TO" in txt and "need NOT agree in every bit" in txt
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    n_args = len(re.search(r"int\s+%s\s*\((.*?)\);" % ENTRY, code, re.S).group(1).split(","))
    assert restype is C.c_int and len(argtypes) == n_args == 27
    h = _lib.lib()
    assert hasattr(h, ENTRY) and _lib.ABI_VERSION == 4 and h.sdirt_abi_version() == 4
    assert h.sdirt_render_layers_grad(None, None, 0, None, None, 0.0, None, None, 0.0, 1, 1, 1, None, 1, None, None,
                                      None, None, 0, 1, 1, 1, None, None, None, 0, None) != 0
    assert b"null lens" in h.sdirt_last_error()


def test_the_new_arguments_are_refused_before_anything_touches_the_gpu():
    from sdirt_amd import _lib
    from sdirt_amd.render_rt import layer_grad_batch, layer_grads_float64
    lens = make_lens("rf50mm", "cpu")
    lens.prepare_sensor(sensor_res=(4, 6), sensor_size=(1.0, 1.5))
    K = len(lens.surfaces)
    img, alpha, zs = torch.zeros(2, 3, 4, 6), torch.ones(2, 4, 6), [-500.0, -1000.0]
    pts = (torch.zeros(2, 4, 6), torch.zeros(2, 4, 6))
    kw = dict(scales=[5.0, 10.0], spp=2, pupil_points=pts)
    # return_sums with a recorded gradient
    for leaf in ("img", "alpha"):
        a, b = img.clone().requires_grad_(leaf == "img"), alpha.clone().requires_grad_(leaf == "alpha")
        with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
            lens.render_layers(a, b, zs, scene_grad=True, return_sums=True, **kw)
    with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
        lens.render_plane(img.clone().requires_grad_(), -500.0, scale=5.0, spp=2, pupil_points=pts, scene_grad=True,
                          return_sums=True)
    # ... but not where nothing is recorded: the call gets as far as asking for the GPU
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img, alpha, zs, scene_grad=True, return_sums=True, **kw)
    with torch.no_grad(), pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img.clone().requires_grad_(), alpha, zs, scene_grad=True, return_sums=True, **kw)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img.clone().requires_grad_(), alpha, zs, return_sums=True, **kw)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_layers(img.clone().requires_grad_(), alpha, zs, scene_grad=True, **kw)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_rgbd(img.clone().requires_grad_(), torch.full((2, 1, 4, 6), -1000.0), spp=2, scales=[10.0],
                         pupil_points=pts, scene_grad=True)
    # layer_grad_batch
    trips, gnum = [1] * K, torch.zeros(1, 3, 4, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="2 layers need 2 depths and 2 scales"):
        layer_grad_batch(lens, alpha, img, zs, [1.0], *pts, trips, gnum)
    with pytest.raises(ValueError, match="strictly descending"):
        layer_grad_batch(lens, alpha, img, zs[::-1], [1.0, 2.0], *pts, trips, gnum)
    with pytest.raises(ValueError, match="pupil points must be"):
        layer_grad_batch(lens, alpha, img, zs, [1.0, 2.0], pts[0], pts[1][:1], trips, gnum)
    with pytest.raises(ValueError, match="trip counts for a lens of"):
        layer_grad_batch(lens, alpha, img, zs, [1.0, 2.0], *pts, trips[:-1], gnum)
    for bad in (gnum.float(), gnum[:, :2], torch.zeros(2, 3, 4, 6, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="gnum must be float64"):
            layer_grad_batch(lens, alpha, img, zs, [1.0, 2.0], *pts, trips, bad)
    with pytest.raises(ValueError, match="both False"):
        layer_grad_batch(lens, alpha, img, zs, [1.0, 2.0], *pts, trips, gnum, galpha=False, gtex=False)
    with pytest.raises(ValueError, match="no coverage gradient"):
        layer_grad_batch(lens, None, img, zs, [1.0, 2.0], *pts, trips, gnum, galpha=torch.zeros(2, 4, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="both False"):
        layer_grad_batch(lens, None, img, zs, [1.0, 2.0], *pts, trips, gnum, gtex=False)
    with pytest.raises(ValueError, match="layers differ"):
        layer_grad_batch(lens, None, img, zs, [1.0], *pts, trips, gnum)
    with pytest.raises(ValueError, match="float32"):
        layer_grad_batch(lens, None, img.double(), zs, [1.0, 2.0], *pts, trips, gnum)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_grad_batch(lens, alpha, img, zs, [1.0, 2.0], *pts, trips, gnum)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_grad_batch(lens, None, img[0], zs[:1], [1.0], *pts, trips, gnum)
    # layer_grads_float64
    land = torch.zeros(3 + 2 * 2, 2, 4, 6)
    with pytest.raises(ValueError, match="landing record of 7 rows"):
        layer_grads_float64(land[:5], alpha, img, [1.0, 2.0], gnum, views=1)
    with pytest.raises(ValueError, match="gnum must be"):
        layer_grads_float64(land, alpha, img, [1.0, 2.0], gnum, views=2)
    with pytest.raises(ValueError, match="alpha has 2 layers"):
        layer_grads_float64(land[:5], alpha, img[0], [1.0], gnum, views=1)
