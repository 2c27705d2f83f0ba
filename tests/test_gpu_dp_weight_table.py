"""The dual-pixel weight table of the fused PSF kernel (sdirt_psf.hip: dp_table_for, k_psf_lr's TAB instantiations).

The Lean small-radius instantiations of k_psf_lr read the segment-area part of a ray's sub-pixel weights (sl, sr) from
a table over x_tan that belongs to the sensor (h, f, w, r) and lives in the lens handle, instead of evaluating
dp_weights_small's six segment-area polynomials.  Checked here: the table against a float64 restatement of
monte_carlo.py:169-206 (it may not be worse than the polynomial it replaces), the kernel end to end with the table on
and off (SDIRT_DP_WEIGHT_TABLE=0 is the hook) and against the oracle, the rebuild when the parameters change, and the
paths that must not notice the table at all."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import load_state, make_lens
from render_rt_f64 import weights_f64

from sdirt_amd import _lib
from sdirt_amd.basics import dptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULT = (0.78, 1.44, 0.3, 0.5)
# the default sensor; a radius that is no power of two (and leaves the +-0.5 clamps of the strip widths apart from the
# +-r clamps of the areas); a small w (the three abscissae of a trio nearly coincide); a large h (f - h small: the
# abscissae through the microlens are twice as steep in x_tan as the default's)
PARAM_SETS = [DEFAULT, (0.78, 1.44, 0.3, 0.4), (0.78, 1.44, 0.02, 0.5), (1.0, 1.44, 0.3, 0.5)]
# steeper still: the library's bound on the interpolation error (0.148 * 1.886 r^2 (z' 2^-k)^1.5, sdirt_psf.hip) passes
# 1e-7 and it declines to build a table
TOO_STEEP = (1.25, 1.44, 0.3, 0.5)
HOOK = "SDIRT_DP_WEIGHT_TABLE"


@contextlib.contextmanager
def table(on):
    old = os.environ.get(HOOK)
    if on:
        os.environ.pop(HOOK, None)
    else:
        os.environ[HOOK] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(HOOK, None)
        else:
            os.environ[HOOK] = old


@pytest.fixture(scope="module")
def lens():
    return make_lens("rf50mm", DEV, load_state("rf50mm"))


def saturation_points(h, f, w, r):
    """Every x_tan at which one clamped argument of the model starts or stops being clamped: (of the segment areas -- what
    the table holds --, of the strip widths)."""
    fmh = f - h
    g, c = f * h / fmh, w * f / fmh
    areas = [(c0 - s * r) / g for c0 in (c, 0.0, -c) for s in (1, -1)]               # microlens trio at +-r
    areas += [(c0 - s * r) / h for c0 in (w, 0.0, -w) for s in (1, -1)]              # pixel trio at +-r
    strips = [(c0 - s * 0.5) / h for c0 in (w, 0.0, -w) for s in (1, -1)]            # ... and at +-0.5
    return np.array(sorted(areas)), np.array(sorted(strips))


def both_forms(lens, dp, x):
    """sdirt_dp_weight_table_selftest: (table-interpolated, closed-form) [n, 2] float64 and (entries, log2 cells per unit)."""
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    tab = torch.empty((xt.numel(), 2), dtype=torch.float32, device=DEV)
    closed = torch.empty_like(tab)
    info = (C.c_int32 * 2)()
    dpp = _lib.DpParams(*[float(v) for v in dp])
    _lib.check(_lib.lib().sdirt_dp_weight_table_selftest(lens.dev_lens(0.589), C.byref(dpp), dptr(xt), xt.numel(), dptr(tab),
                                                        dptr(closed), info, stream_ptr(lens.device)))
    torch.cuda.synchronize()
    return tab.cpu().numpy().astype(np.float64), closed.cpu().numpy().astype(np.float64), (int(info[0]), int(info[1]))


def table_errors(lens, dp):
    """max |table - float64| and max |closed form - float64| over 2e5 abscissae: the whole table and beyond it, and a
    dense cluster within +-3 cells of every saturation point."""
    rng = np.random.default_rng(5)
    _, _, (entries, k) = both_forms(lens, dp, np.zeros(1))
    cell, X = 2.0 ** -k, (entries - 1) / 2 * 2.0 ** -k
    areas, strips = saturation_points(*dp)
    assert np.abs(areas).max() < X - cell, "the table ends before the last saturation point of an area"
    sat = np.unique(np.concatenate([areas, strips]))
    near = (sat[:, None] + rng.uniform(-3, 3, (sat.size, 4000)) * cell).ravel()
    reach = 1.25 * max(X, np.abs(strips).max())
    wide = rng.uniform(-reach, reach, 200_000 - near.size - 8)
    far = np.array([-1e9, -1e3, -reach - cell, -reach, reach, reach + cell, 1e3, 1e9])
    x = np.concatenate([near, wide, far]).astype(np.float32)
    assert x.size == 200_000 and np.sum(np.abs(x) > X) > 1000 and np.sum(np.abs(x) > reach) >= 4
    tab, closed, _ = both_forms(lens, dp, x)
    want = np.stack(weights_f64(x, *dp), -1)
    e_tab, e_closed = np.abs(tab - want).max(), np.abs(closed - want).max()
    # beyond the table the index is clamped: the end entries are the saturated values
    ends = tab[-8:]
    assert np.array_equal(ends[0], ends[1]) and np.array_equal(ends[1], ends[2]) and np.array_equal(ends[2], ends[3])
    assert np.array_equal(ends[4], ends[5]) and np.array_equal(ends[5], ends[6]) and np.array_equal(ends[6], ends[7])
    assert np.abs(ends - want[-8:]).max() <= 2.0 ** -23, np.abs(ends - want[-8:]).max()
    return e_tab, e_closed, entries, k


@pytest.fixture(scope="module")
def default_bound(lens):
    """What test 1 bounds the table's error by on the default sensor: the closed form's own error against float64."""
    return table_errors(lens, DEFAULT)[1]


@pytest.mark.parametrize("dp", PARAM_SETS)
def test_table_is_no_worse_than_the_polynomial_it_replaces(lens, dp):
    e_tab, e_closed, entries, k = table_errors(lens, dp)
    print(f"(h, f, w, r) = {dp}: {entries} entries, cell 2^-{k}: max |table - f64| {e_tab:.3e}, "
          f"max |dp_weights_small<Lean> - f64| {e_closed:.3e}")
    assert e_tab <= e_closed * 1.0, (dp, e_tab, e_closed)


def test_a_sensor_too_steep_for_the_bound_keeps_the_closed_form(lens):
    with pytest.raises(_lib.SdirtError, match="no weight table"):
        both_forms(lens, TOO_STEEP, np.zeros(4))
    a, b = _on_and_off(lambda: _call(lens, TOO_STEEP))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- the kernel, end to end
def _uniforms(spp, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, spp, generator=g).numpy(), torch.rand(2, 2048, generator=g).numpy()


@pytest.fixture(scope="module")
def focus_depth(lens):
    """The depth whose on-axis PSF is the most concentrated of a coarse sweep: a point near the focal plane."""
    depths = [-600.0, -900.0, -1200.0, -1500.0, -2000.0, -3000.0, -5000.0, -10000.0, -20000.0]
    torch.manual_seed(3)
    L, _ = lens.psf_lr(torch.tensor([[0.0, 0.0, z] for z in depths]), ks=21, spp=512, normalize=False)
    return depths[int(L.amax(dim=(1, 2)).argmax())]


@pytest.fixture(scope="module")
def oracle_psfs(oracle, focus_depth):
    """The three points and, per (ks, spp), their pupil samples and the oracle's PSFs: computed once."""
    st = load_state("rf50mm")
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.95, -0.95, -3000.0], [0.2, 0.1, focus_depth]])
    out = {}
    oracle.set_num_threads(8)
    for ks, spp in [(21, 1024), (65, 1024), (21, 4096)]:
        u, uc = _uniforms(spp)
        x2, y2 = oracle.pupil_samples(u[0], u[1], st["pupil_r"])
        xc, yc = oracle.pupil_samples(uc[0], uc[1], st["pupil_r"] * 0.25)
        lo, ro, _, ok = oracle.psf(st, pts.numpy(), x2, y2, xc, yc, ks, dp=list(DEFAULT))
        assert ok
        out[ks, spp] = ((x2, y2), (xc, yc), lo, ro)
    return pts, out


# Which sums of a call do not depend on the order the waves reach them in.  The tiles of ks 21, and of ks 65 without R,
# are float64 (plan_psf): every order rounds to the same float32.  ks 65 with R -- the instantiation the benchmark's
# headline runs -- has float32 tiles, whose LDS atomics commute only up to a rounding per addition, so two calls of the
# SAME build differ by a few 1e-7 of the peak, as much as the bound allows the table.  That case is asserted twice:
#   with lens.deterministic (float64 tiles in 1024-thread workgroups, the TAB instantiation of that form) at the bound
#       alone: the difference is the table's and nothing else's;
#   with the float32 tiles at the bound plus an allowance for the order of the sums, measured in the test itself on the
#       code the table does not touch: three calls with the table OFF, the largest of their three pairwise gaps, twice.
#       On against off holds one draw of the same noise (a gap of two independent calls, whichever kernel made them);
#       each gap is a maximum over 3 x 2 x 65 x 65 pixels and scatters little from pair to pair, twice the largest of
#       three is out of its reach, and is still some 1e-7: a table path wrong by 1e-6 of the peak fails.
# (21, 4096) is a case of this file's own: three points cut along spp -- four workgroups per point, the chief-ray pass a
# launch of its own, the !CENTER instantiations.  The four partial grids of a point meet in global float32 atomics:
# three roundings of at most 2^-24 of the peak per call in the pixel and as many in the peak it is divided by, in
# each of the two calls: 12 * 2^-24 on top of the bound.
SUM_ORDER = {(21, 4096): 12 * 2.0 ** -24}


@pytest.mark.parametrize("ks,spp,want_r", [(21, 1024, True), (21, 1024, False), (65, 1024, True), (65, 1024, False),
                                           (21, 4096, True)])
def test_kernel_with_the_table_against_the_closed_form_and_the_oracle(lens, oracle_psfs, default_bound, ks, spp, want_r):
    pts, cases = oracle_psfs
    pxy, cxy, lo, ro = cases[ks, spp]
    float_tiles = ks == 65 and want_r

    def both(deterministic):
        lens.deterministic = deterministic
        try:
            return _on_and_off(lambda: lens.psf_lr(pts, ks=ks, dp=DEFAULT, want_r=want_r, pupil_xy=pxy, center_pupil_xy=cxy))
        finally:
            lens.deterministic = False

    sides = [0, 1] if want_r else [0]
    gap = lambda a, b: max(float((a[s] - b[s]).abs().max()) for s in sides)
    to_oracle = lambda a: max(float(np.abs(a[s].cpu().numpy() - (lo, ro)[s]).max()) for s in sides)
    on, off = both(float_tiles)
    assert want_r or on[1] is None
    # both calls normalise each PSF to its peak; a ray's weight moves by at most the table's plus the closed form's
    # error, each bounded by test 1's bound, on taps of at most 1
    largest_tap = 1.0
    tol = 2.0 * default_bound * largest_tap + SUM_ORDER.get((ks, spp), 0.0)
    d, d_or = gap(on, off), to_oracle(on)
    print(f"ks {ks} spp {spp} R {want_r}: max |table - closed form| {d:.3e} of the peak (bound {tol:.3e})")
    print(f"ks {ks} spp {spp} R {want_r}: max |table - oracle| {d_or:.3e}")
    if float_tiles:
        on32, off32 = both(False)
        with table(False):
            offs = [off32] + [lens.psf_lr(pts, ks=ks, dp=DEFAULT, want_r=want_r, pupil_xy=pxy, center_pupil_xy=cxy) for _ in range(2)]
        order = 2.0 * max(gap(offs[i], offs[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
        d32, d_or32 = gap(on32, off32), to_oracle(on32)
        print(f"ks {ks} spp {spp} R {want_r}, float32 tiles: max |table - closed form| {d32:.3e} (bound {tol:.3e} + order of "
              f"the sums {order:.3e}), max |table - oracle| {d_or32:.3e}")
        assert order <= 1e-6, order                 # the allowance stays what it is meant for: roundings of float32 sums
        assert d32 <= tol + order, (d32, tol, order)
        d_or = max(d_or, d_or32)
    assert d <= tol, (d, tol)
    assert d_or <= 5e-6, d_or          # tests/test_gpu_parity.py::test_random_points_fused_vs_oracle


# ------------------------------------------------------------------------------------------------------- invalidation
def _call(lens_, dp, ks=21, spp=1024):
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.6, -0.5, -1200.0], [-0.3, 0.4, -4000.0]])
    st = load_state("rf50mm")
    from oracle import oracle as orc
    u, uc = _uniforms(spp, seed=12)
    pxy = orc.pupil_samples(u[0], u[1], st["pupil_r"])
    cxy = orc.pupil_samples(uc[0], uc[1], st["pupil_r"] * 0.25)
    with torch.no_grad():
        return lens_.psf_lr(pts, ks=ks, dp=dp, pupil_xy=pxy, center_pupil_xy=cxy)


def _same(a, b, tol=1.2e-7):
    return all(float((x - y).abs().max()) <= tol for x, y in zip(a, b))


def test_other_parameters_rebuild_the_table(lens):
    A, B = DEFAULT, (0.70, 1.50, 0.25, 0.45)
    fresh = {dp: _call(make_lens("rf50mm", DEV, load_state("rf50mm")), dp) for dp in (A, B)}
    assert not _same(fresh[A], fresh[B], 1e-3)
    for dp in (A, B, A):
        got = _call(lens, dp)
        assert _same(got, fresh[dp]), dp
    # a parameter changed in place between two calls
    h = torch.tensor(0.78, requires_grad=True)
    first = _call(lens, (h, 1.44, 0.3, 0.5))
    with torch.no_grad():
        h.add_(0.05)
    second = _call(lens, (h, 1.44, 0.3, 0.5))
    assert _same(first, fresh[A])
    assert _same(second, _call(make_lens("rf50mm", DEV, load_state("rf50mm")), (float(h), 1.44, 0.3, 0.5)))
    assert not _same(first, second, 1e-3)


# ----------------------------------------------------------------------------------------------------- untouched paths
def _on_and_off(fn):
    out = []
    for on in (True, False):
        with table(on):
            out.append(fn())
    return out


def test_strict_ieee_calls_do_not_see_the_table():
    ieee = make_lens("rf50mm", DEV, load_state("rf50mm"))
    ieee.precision = "ieee"
    a, b = _on_and_off(lambda: _call(ieee, DEFAULT))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_big_radius_calls_do_not_see_the_table(lens):
    """r = 0.7 accumulates in float32 tiles whatever ks is, and two calls of one build agree bit for bit only where the
    order of the additions is fixed: 64 rays per point are ONE wave's, added in program order."""
    a, b = _on_and_off(lambda: _call(lens, (0.78, 1.44, 0.3, 0.7), spp=64))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool((x.sum(dim=(1, 2)) > 0).all()) for x in a)                          # rays did land, at every point


def test_backward_does_not_see_the_table(lens):
    """The shape of tests/test_gpu_dp_grad.py's DP-parameter gradient tests: values and gradients of a differentiable call."""
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.35, -0.2, -1200.0], [-0.6, 0.45, -2500.0]])
    st = load_state("rf50mm")
    from oracle import oracle as orc
    u, uc = _uniforms(1024, seed=27)
    pxy = orc.pupil_samples(u[0], u[1], st["pupil_r"])
    cxy = orc.pupil_samples(uc[0], uc[1], st["pupil_r"] * 0.25)
    G = torch.randn((3, 21, 21), generator=torch.Generator().manual_seed(27)).to(DEV)

    def run():
        leaves = [torch.tensor(v, requires_grad=True) for v in DEFAULT[:3]]
        L, R = lens.psf_lr(pts, ks=21, dp=(*leaves, 0.5), pupil_xy=pxy, center_pupil_xy=cxy)
        ((L * G).sum() + (R * G.flip(0)).sum()).backward()
        return [L.detach(), R.detach()] + [t.grad for t in leaves]

    a, b = _on_and_off(run)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
