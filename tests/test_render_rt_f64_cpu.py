"""The product's float64 restatement of the plane render's lookup and sums (render_rt.plane_sums_float64, torch)
against the independent one (tests/render_rt_f64.py, numpy, written from DESIGN.md §7o) on synthetic landings: the
texture shapes of tests/test_gpu_render_raytraced_edges.py, landings reaching 1.5 x the texture's half extent on either
axis, a fifth of the rays dead and some of those carrying NaN, +-inf and +-3e38, fractional weights, one and two views.

Both evaluate the same S float64 terms per element and may sum them in different orders: they must agree within
2 S 2^-53 sum|term| (render_rt_f64's docstring), the bound the GPU tests use for the kernel."""
import numpy as np
import pytest
import torch

import render_rt_f64 as R

TEX_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 141), (11, 280)]
H, W = 3, 37
FLOOR = 0.05                                                 # of the live rays, in every class a texture extent has


def synthetic(Ht, Wt, S, seed):
    """-> px, py, ra [S, H, W], w [2, S, H, W] fp32, tex [3, Ht, Wt] fp32, inv_texel.  u = Wt/2 - px inv is uniform on
    Wt/2 -+ 0.75 Wt: the first tap's column is < 0 where u < 0.5 and >= Wt - 1 where u >= Wt - 0.5, (0.25 Wt + 0.5) /
    (1.5 Wt) of the rays each (0.5 for Wt = 1, 0.19 for Wt = 280); rows alike."""
    rng = np.random.default_rng(seed)
    inv = 0.37 * (1 + Wt) ** 0.5                             # texels per mm: no power of two, the products round
    px = rng.uniform(-1.5, 1.5, (S, H, W)) * (Wt / 2) / inv
    py = rng.uniform(-1.5, 1.5, (S, H, W)) * (Ht / 2) / inv
    ra = (rng.uniform(size=(S, H, W)) >= 0.2).astype(np.float32)
    w = rng.uniform(0.0, 1.0, (2, S, H, W)).astype(np.float32)
    px, py = px.astype(np.float32), py.astype(np.float32)
    dead = np.flatnonzero(ra == 0)
    specials = [np.nan, np.inf, -np.inf, 3e38, -3e38]
    for n, idx in enumerate(dead[::2]):                      # every other dead ray lands nowhere sensible
        px.flat[idx] = specials[n % 5]
        py.flat[idx] = specials[(n // 5) % 5]
    tex = rng.uniform(-0.25, 0.75, (3, Ht, Wt)).astype(np.float32)
    return px, py, ra, w, tex, inv


@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("S", [8, 5])
@pytest.mark.parametrize("Ht, Wt", TEX_SHAPES)
def test_the_product_s_restatement_equals_the_independent_one(Ht, Wt, S, views):
    from sdirt_amd.render_rt import plane_sums_float64
    px, py, ra, w, tex, inv = synthetic(Ht, Wt, S, seed=1000 * Ht + Wt + S)
    live = ra != 0
    dead_share = 1 - live.mean()
    assert 0.1 < dead_share < 0.3, dead_share
    for special in (np.isnan, np.isposinf, np.isneginf, lambda a: a == np.float32(3e38), lambda a: a == np.float32(-3e38)):
        assert special(px[~live]).any() and special(py[~live]).any()
        assert not special(px[live]).any() and not special(py[live]).any()
    # every class of landing a texture of this extent has, on either axis, holds its share of the live rays
    c0, r0, fu, fv = R.tap_origin(np.where(live, px, 0), np.where(live, py, 0), inv, Ht, Wt)
    for axis, first, n in (("x", c0, Wt), ("y", r0, Ht)):
        lo, mid, hi = R.tap_classes(first, n, live)
        print(f"tex {Ht} x {Wt}, S {S}: {axis} classes  < 0: {lo:.3f}   0..n-2: {mid:.3f}   >= n-1: {hi:.3f}")
        assert lo >= FLOOR and hi >= FLOOR, (axis, lo, mid, hi)
        assert mid >= FLOOR if n > 1 else mid == 0, (axis, lo, mid, hi)       # one texel: no tap pair inside
    assert float(fu[live].min()) >= 0 and float(fu[live].max()) < 1 and 0.2 < float(fu[live].mean()) < 0.8

    num, den, ab = R.plane_sums_f64(px, py, ra, w[:views], tex, inv)
    assert num.shape == (views, 3, H, W) and den.shape == (views, H, W) and num.dtype == den.dtype == np.float64
    landing = torch.from_numpy(np.concatenate((np.stack((px, py, ra)), w)))
    pnum, pden, pab = plane_sums_float64(landing, torch.from_numpy(tex), inv, views=views, return_abs=True)
    pnum, pden, pab = pnum.numpy(), pden.numpy(), pab.numpy()
    assert np.isfinite(num).all() and np.isfinite(pnum).all() and np.isfinite(den).all() and np.isfinite(pden).all()
    eps = R.sum_bound(S)
    worst = float((np.abs(num - pnum) / np.maximum(eps * ab, 1e-300)).max())
    print(f"tex {Ht} x {Wt}, S {S}, views {views}: worst |num - product's| / bound {worst:.3f}")
    assert (np.abs(num - pnum) <= eps * ab).all(), worst
    assert (np.abs(den - pden) <= eps * den).all()             # the terms of den are w ra >= 0: sum|term| is den
    assert (np.abs(ab - pab) <= eps * ab).all()
    assert (den > 0).any() and (ab > 0).any()


def test_the_restatement_on_a_landing_worked_by_hand():
    """One pixel, a 2 x 3 texture, 1 texel per mm, three rays: at the texture's centre between the four texels of
    columns 1 and 2 (px = -0.5: u = 2, a = 1.5, c0 = 1, fu = 0.5; py = 0: v = 1, b = 0.5, r0 = 0, fv = 0.5), far out to
    the top left (+x on the plane is the texture's left, -y its top: the texel (0, 0) alone) and a dead one on NaN."""
    tex = np.array([[[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]]], np.float32)
    px = np.array([-0.5, 50.0, np.nan], np.float32).reshape(3, 1, 1)
    py = np.array([0.0, -50.0, np.inf], np.float32).reshape(3, 1, 1)
    ra = np.array([1.0, 1.0, 0.0], np.float32).reshape(3, 1, 1)
    w = np.array([[0.5, 0.25, 0.75], [1.0, 1.0, np.nan]], np.float32).reshape(2, 3, 1, 1)
    num, den, ab = R.plane_sums_f64(px, py, ra, w, tex, 1.0)
    centre = 0.25 * (2.0 + 4.0 + 16.0 + 32.0)
    assert num[:, 0, 0, 0].tolist() == [0.5 * centre + 0.25 * 1.0, centre + 1.0]
    assert den[:, 0, 0].tolist() == [0.75, 2.0] and np.array_equal(ab, num)
    c0, r0, fu, fv = R.tap_origin(px[:2], py[:2], 1.0, 2, 3)
    assert c0.flatten().tolist() == [1.0, -49.0] and r0.flatten().tolist() == [0.0, -50.0]
    assert fu.flatten().tolist() == [0.5, 0.0] and fv.flatten().tolist() == [0.5, 0.5]
    assert R.tap_classes(c0, 3, np.ones(c0.shape, bool)) == (0.5, 0.5, 0.0)
