"""Object-point gradients without a GPU: the C ABI declares the new entry, the float64 restatement (tests/point_f64.py)
agrees with central differences of its own forward and, where the reference checkout is present, with the reference's own
float64 autograd (tools/gen_point_grad.py); the library's chain from dLoss/d(point_obj) to dLoss/d(points) is autograd's of
optics.py:956-960; the keyword's plain path and its refusals."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import point_f64 as P
import trace_f64 as T
from conftest import make_lens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "sdirt_trace2sensor_grad_points"


def test_header_declares_the_entry_and_the_library_exports_it():
    import ctypes as C
    from sdirt_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    h = _lib.lib()
    assert re.search(r"\b%s\s*\(" % ENTRY, code)
    assert ENTRY in _lib.SIGNATURES and hasattr(h, ENTRY)
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert restype is C.c_int and len(argtypes) == 15
    assert "optics.py:460-494, 889-904, 956-960" in txt
    assert h.sdirt_abi_version() == 4
    # a null argument is refused before anything touches a device
    assert h.sdirt_trace2sensor_grad_points(None, None, 0, 0.0, None, None, None, 4, 1, None, None, 0.0, None, 1, None) != 0


def _setup(name, n_rays=48, seed=1):
    """A lens, two field points and a bundle of pupil points well inside the first surface (every ray stays valid)."""
    lens = make_lens(name, "cpu")
    consts = (float(np.tan(lens.hfov)), float(lens.r_last), float(lens.sensor_size[1]), float(lens.sensor_size[0]))
    g = torch.Generator().manual_seed(seed)
    pupil_z, pupil_r = lens.entrance_pupil()
    rad = torch.rand(n_rays, generator=g).sqrt() * float(pupil_r) * 0.6
    ang = torch.rand(n_rays, generator=g) * 2 * np.pi
    x2, y2 = (rad * ang.cos()).float(), (rad * ang.sin()).float()
    pts = torch.tensor([[0.35, -0.2, -1500.0], [-0.5, 0.4, -800.0]], dtype=torch.float64)
    table, theta = T.lens_table(lens, 0.589), lens.surface_parameters().double()
    return lens, consts, pts, x2, y2, float(pupil_z), table, theta


def _check_against_differences(f, pts, label):
    """autograd of the scalar f(points) against central differences: the bar is the quotient's own truncation error,
    estimated by halving the step (|q(h) - q(h / 2)|: the error of q(h) is 4/3 of it for a smooth f), times 2."""
    p = pts.clone().requires_grad_()
    f(p).backward()
    for n in range(pts.shape[0]):
        for c, h in ((0, 2e-3), (1, 2e-3), (2, 2.0)):          # normalised x, y; depth in mm
            def quotient(step):
                lo, hi = pts.clone(), pts.clone()
                lo[n, c] -= step
                hi[n, c] += step
                with torch.no_grad():
                    return float(f(hi) - f(lo)) / (2 * step)
            q1, q2 = quotient(h), quotient(h / 2)
            bar = 2 * abs(q1 - q2)
            got = float(p.grad[n, c])
            print(f"{label} point {n} component {c}: autograd {got:.9e} quotient {q2:.9e} bar {bar:.2e}")
            assert got != 0 and bar < 1e-3 * abs(got), (got, bar)
            assert abs(q2 - got) <= bar, (n, c, got, q2, bar)


@pytest.mark.parametrize("name", ["rf50mm", "rf35mm"])
def test_restatement_gradients_match_central_differences_of_its_own_forward(name):
    lens, consts, pts, x2, y2, pupil_z, table, theta = _setup(name)
    K, S, N = len(lens.surfaces), len(x2), pts.shape[0]
    g = torch.Generator().manual_seed(2)
    rg = torch.randn(4, N * S, generator=g).double()

    def linear(p):
        terms = P.linear_form(P.object_points(p, *consts), x2, y2, pupil_z, theta, table, [5] * K, lens.d_sensor, rg, None)
        assert bool(torch.isfinite(terms).all())
        return terms.sum()
    _check_against_differences(linear, pts, f"{name} linear form")
    w = torch.randn(N, 2, generator=g).double()
    ra = torch.ones(N * S)

    def centre(p):
        c = P.centre(P.object_points(p, *consts), x2 * 0.25, y2 * 0.25, pupil_z, theta, table, [5] * K, lens.d_sensor, ra)
        return (c * w).sum()
    _check_against_differences(centre, pts, f"{name} centre")
    # per-ray copies of the points give the same total
    p = pts.clone().requires_grad_()
    linear(p).backward()
    each = P.object_points(pts, *consts).unsqueeze(1).expand(N, S, 3).clone().requires_grad_()
    P.linear_form(each, x2, y2, pupil_z, theta, table, [5] * K, lens.d_sensor, rg, None).sum().backward()
    np.testing.assert_allclose(P.chain(pts, each.grad.sum(1), *consts).numpy(), p.grad.numpy(), rtol=1e-10, atol=1e-12)
    # ... also through the library's chain (trace_grad.points_chain), which is what the backward applies
    from sdirt_amd.trace_grad import PointSamples, points_chain
    np.testing.assert_allclose(points_chain(pts, each.grad.sum(1), PointSamples(None, None, pupil_z, *consts)).numpy(),
                               p.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_library_chain_is_autograd_of_the_pinhole_scale():
    """trace_grad.points_chain against autograd of the three lines of optics.py:956-960 in float64."""
    from sdirt_amd.trace_grad import PointSamples, points_chain
    lens = make_lens("rf50mm", "cpu")
    consts = (float(np.tan(lens.hfov)), float(lens.r_last), float(lens.sensor_size[1]), float(lens.sensor_size[0]))
    g = torch.Generator().manual_seed(3)
    pts = torch.cat((torch.rand(7, 2, generator=g) * 2 - 1, -300.0 - 20000.0 * torch.rand(7, 1, generator=g)), 1)
    p_bar = torch.randn(7, 3, generator=g, dtype=torch.float64)
    p = pts.double().requires_grad_()
    depth = p[:, 2]
    scale = -depth * consts[0] / consts[1]
    point_obj = p.clone()
    point_obj[..., 0] = p[..., 0] * scale * consts[2] / 2
    point_obj[..., 1] = p[..., 1] * scale * consts[3] / 2
    (point_obj * p_bar).sum().backward()
    smp = PointSamples(None, None, 0.0, *consts)
    got = points_chain(pts, p_bar, smp)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), p.grad.numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(P.chain(pts.double(), p_bar, *consts).numpy(), p.grad.numpy(), rtol=1e-14, atol=0)
    assert torch.equal(P.object_points(pts.double(), *consts), point_obj.detach())


needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")


@needs_reference
def test_restatement_matches_reference_float64_gradients_in_the_points():
    """Both centre rules, r = 0.5 and 0.65, both directions, both lenses, a field corner at 0.3 m and at 20 m each: the
    reference's own float64 autograd of sum(G * forward_integral(...)) in `points` (tools/gen_point_grad.py) to 1e-9
    relative.  With center=True the rays' term and the centre's cancel to a few percent of either, and an entry that
    cancels is rounding noise of the float64 sums on both sides: the atol is 1e-12 of the sum of the per-ray
    magnitudes, as test_trace_grad_cpu.py has 1e-12 of the largest entry for the entries that vanish by symmetry."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_point_grad as gen
    cases = gen.cases()
    assert len(cases) == 8 and {c["r"] for c in cases} == {0.5, 0.65} and {c["direct"] for c in cases} == {"l", "r"} and {c["center"] for c in cases} == {True, False}
    assert {(c["lens"], bool(c["point"][2] > -1000)) for c in cases} == {(n, near) for n in ("rf50mm", "rf35mm") for near in (True, False)}
    from sdirt_amd.trace_grad import PointSamples, points_chain
    for c in cases:
        # the generator's chain is the library's
        bar = torch.tensor([[0.3, -1.1, 0.7]], dtype=torch.float64)
        smp = PointSamples(None, None, c["pupil_z"], c["tan_hfov"], c["r_last"], c["sensor_w"], c["sensor_h"])
        np.testing.assert_allclose(points_chain(torch.from_numpy(c["point"]).reshape(1, 3), bar, smp)[0].numpy(),
                                   gen.chain(c, bar[0].numpy()), rtol=1e-14)
        total, mag = gen.restated(c, per_ray=True)
        plain = gen.restated(c)
        print(f"{c['lens']} {c['point'].tolist()} center {c['center']} r {c['r']} {c['direct']}: "
              f"|restatement - g64| / |g64| = {np.abs(plain - c['grad64']) / np.abs(c['grad64'])}, / sum|terms| = "
              f"{np.abs(plain - c['grad64']) / mag}")
        assert bool((np.abs(plain - c["grad64"]) <= 1e-9 * np.abs(c["grad64"]) + 1e-12 * mag).all())
        assert bool((np.abs(total - plain) <= 1e-9 * np.abs(plain) + 1e-12 * mag).all())


def test_point_grad_without_a_gradient_is_the_plain_call():
    lens = make_lens("rf50mm", "cpu")
    seen = []
    lens._psf_lr = lambda *a, **k: seen.append("plain") or ("plain", None)
    lens._psf_lr_grad = lambda *a, **k: seen.append(("grad", k)) or ("grad", None)
    pts = torch.tensor([[0.1, 0.2, -1500.0]])
    assert lens.psf_lr(pts, point_grad=True)[0] == "plain"                              # needs no gradient
    with torch.no_grad():
        assert lens.psf_lr(pts.clone().requires_grad_(), point_grad=True)[0] == "plain"  # grad mode off
    assert lens.psf_lr(pts.clone().requires_grad_())[0] == "plain"                      # the default: center=True gives none
    assert lens.psf_lr(pts.clone().requires_grad_(), point_grad=True)[0] == "grad"
    assert lens.psf_lr(pts.clone().requires_grad_(), center=False, point_grad=True)[0] == "grad"
    assert seen[-1][1].get("point_grad") is True and seen[-2][1].get("point_grad") is True
    assert lens.psf_lr(pts.clone().requires_grad_(), center=False)[0] == "grad"         # the pinhole-centre term alone, as before
    assert "point_grad" not in seen[-1][1]
    assert lens.psf_diff(pts.clone().requires_grad_(), point_grad=True) == "grad" and seen[-1][1].get("point_grad") is True
    assert lens.psf_diff(pts, point_grad=True) == "plain"


@pytest.mark.parametrize("kw", [dict(defer=True), dict(out="x"), dict(center_out="x"), "adaptive"])
def test_point_grad_refusals(kw):
    lens = make_lens("rf50mm", "cpu")
    pts = torch.tensor([[0.1, 0.2, -1500.0]], requires_grad=True)
    if kw == "adaptive":
        lens.trip_policy = "adaptive"
        kw = {}
    with pytest.raises(ValueError):
        lens.psf_lr(pts, point_grad=True, **kw)
