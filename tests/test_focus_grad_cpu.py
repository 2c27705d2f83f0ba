"""The gradient of dual-pixel PSFs in the sensor position without a GPU: the float64 restatement (tests/focus_f64.py)
against the reference's own float64 autograd with lens.d_sensor a tensor (computed afresh by tools/gen_focus_grad.py
where the reference checkout is present), with the chief-ray centre detached (the reference as it ships) and in the
graph (the rule of DESIGN.md 7h); the restatement against central differences of its own forward on PSFs that lie
inside the window; and the rules that decide what a `d_sensor=` argument does to a psf call."""
import os
import sys

import numpy as np
import pytest
import torch

import focus_f64 as F
from conftest import load_state

from sdirt_amd import optics
from sdirt_amd.optics import Lensgroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference"),
                                     reason="needs the reference checkout (build container only)")


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_focus_grad
    return gen_focus_grad


@pytest.fixture(scope="module")
def ref_lens(gen):
    return gen.gg.build_lens("rf50mm")


def _t(arrays):
    return None if arrays is None else [torch.from_numpy(a) for a in arrays]


def _restated(case, G, dp, direct, centre_in_graph, square=False, s=None):
    """(loss, dloss/ds) of the restatement on a reference run's float64 bundles (window tested in float64, as there)."""
    ps = load_state("rf50mm")["pixel_size"]
    ks = G.shape[-1]
    leaf = torch.tensor(case["s0"] if s is None else s, dtype=torch.float64, requires_grad=True)
    psf = F.psf(_t(case["rays"]), _t(case["chief"]), leaf, case["s0"], ps, ks, dp, direct,
                pinhole=case["centre"], centre_in_graph=centre_in_graph, mask_dtype=torch.float64)
    loss = (torch.from_numpy(G).double() * psf).sum()
    if square:
        loss = loss + (psf ** 2).sum()
    loss.backward()
    return float(loss), float(leaf.grad), psf.detach().numpy()


@needs_reference
def test_restatement_matches_reference_float64_autograd_centre_detached_and_in_graph(gen, ref_lens):
    """rf50mm; r 0.5 and 0.65; direct l and r; center True and False.  1e-9 relative (the bar of 7d / 7f for a
    restatement against the reference).  With center=True both forms of the centre."""
    assert {c[0] for c in gen.CASES} == {0.5, 0.65} and {c[1] for c in gen.CASES} == {"l", "r"}
    assert {c[2] for c in gen.CASES} == {True, False}
    rng = np.random.default_rng(gen.SEED)
    seen = []
    for r, direct, center in gen.CASES:
        G = rng.standard_normal((len(gen.POINTS), gen.KS, gen.KS)).astype(np.float32)
        for in_graph in ((False, True) if center else (False,)):
            ref = gen.run(ref_lens, gen.POINTS, r, direct, center, G, in_graph)
            loss, grad, psf = _restated(ref, G, (*gen.DP, r), direct, in_graph)
            print(f"r {r} direct {direct} center {center} centre in graph {in_graph}: reference {ref['grad']:+.12e} "
                  f"restatement {grad:+.12e} (relative {abs(grad / ref['grad'] - 1):.1e})")
            assert np.isfinite(ref["grad"]) and ref["grad"] != 0.0
            assert np.abs(psf - ref["psf"]).max() < 1e-9
            np.testing.assert_allclose(grad, ref["grad"], rtol=1e-9, atol=0)
            seen.append((center, in_graph, ref["grad"]))
    # the centre's motion is not a correction: it changes the gradient at first order
    by = {(c, g): v for c, g, v in seen[:2]}
    assert abs(by[(True, True)] - by[(True, False)]) > 0.1 * abs(by[(True, False)])


@needs_reference
def test_rule_has_the_sign_and_size_of_central_differences_where_the_psfs_lie_inside_the_window(gen, ref_lens):
    """The issue's probe in float64: four points whose blur stays inside the 21-pixel window (no ray crosses the
    window mask, a discontinuity finite differences see and no graph does), center=True, loss sum(G psf) + sum(psf^2).
    The restatement's autograd with the centre in the graph has the sign of the central differences of its own forward
    (steps 1e-2, 3e-3, 1e-3 mm) and lies within 5 % of each; with the centre detached -- what the reference's graph gives
    -- the sign is the opposite.  Measured (float64): see DESIGN.md 7h."""
    p = gen.PROBE
    pts = gen.probe_points(ref_lens)
    G = np.random.default_rng(5).standard_normal((len(pts), p["ks"], p["ks"])).astype(np.float32)
    dp, direct = tuple(p["param_list"][:4]), p["param_list"][4]
    ref = gen.run(ref_lens, pts, dp[3], direct, True, G, True, ks=p["ks"], spp=p["spp"], seed=p["seed"], dp=dp[:3],
                  square=True)
    # inside the window: every live ray is inside at s0 and at the outermost finite-difference positions
    ps = load_state("rf50mm")["pixel_size"]
    lim = (p["ks"] / 2 - 0.5) * ps - 0.01 * ps
    rays, chief = _t(ref["rays"]), _t(ref["chief"])
    for s in (ref["s0"] - 1e-2, ref["s0"], ref["s0"] + 1e-2):
        x, y = F.sensor_points(*rays[:5], s, ref["s0"])
        c = F.chief_centre(*chief, s, ref["s0"])
        live = rays[5] != 0
        assert float(((-x - c[:, 0]).abs()[live]).max()) < lim and float(((-y - c[:, 1]).abs()[live]).max()) < lim
    loss, grad, _ = _restated(ref, G, dp, direct, True, square=True)
    _, detached, _ = _restated(ref, G, dp, direct, False, square=True)
    np.testing.assert_allclose(grad, ref["grad"], rtol=1e-9)
    print(f"dloss/ds: centre in graph {grad:+.4f}, centre detached {detached:+.4f}")
    for step in (1e-2, 3e-3, 1e-3):
        up = _restated(ref, G, dp, direct, True, square=True, s=ref["s0"] + step)[0]
        dn = _restated(ref, G, dp, direct, True, square=True, s=ref["s0"] - step)[0]
        fd = (up - dn) / (2 * step)
        print(f"  central difference, step {step:g} mm: {fd:+.4f} (autograd / fd - 1 = {grad / fd - 1:+.2%})")
        assert np.sign(fd) == np.sign(grad) and abs(grad / fd - 1) <= 0.05
        assert np.sign(detached) == -np.sign(fd)


def test_slope_terms_are_the_autograd_terms_of_the_centre():
    """chief_slope_terms (what the kernel test sums) against autograd through chief_centre with per-ray leaves."""
    g = torch.Generator().manual_seed(2)
    Sc, N = 300, 3
    o = [torch.randn((Sc, N), generator=g).float() for _ in range(2)]
    d = torch.nn.functional.normalize(torch.randn((Sc, N, 3), generator=g) * torch.tensor([0.2, 0.2, 0.0])
                                      + torch.tensor([0.0, 0.0, 1.0]), dim=-1).float()
    ra = (torch.rand((Sc, N), generator=g) > 0.2).float()
    d[..., 2][ra == 0] = 0.0                                   # a dead ray's direction is anything: no NaN may leak
    s = torch.full((Sc, N), 62.25, dtype=torch.float64, requires_grad=True)
    c = F.chief_centre(*o, d[..., 0], d[..., 1], d[..., 2], ra, s, 62.25)
    terms = F.chief_slope_terms(d[..., 0], d[..., 1], d[..., 2], ra)
    den = ra.double().sum(0) + 1e-9
    for k in range(2):
        (grad,) = torch.autograd.grad(c[:, k].sum(), s, retain_graph=True)
        assert torch.isfinite(grad).all()
        torch.testing.assert_close(grad, -terms[..., k] / den, rtol=1e-14, atol=0)


# ------------------------------------------------------------------ what d_sensor= does to a psf call
def _routing_lens(monkeypatch, raises=False):
    lens = Lensgroup.__new__(Lensgroup)
    lens.d_sensor = 62.25
    seen = []

    def plain(self, *a):
        seen.append(("plain", self.d_sensor))
        if raises:
            raise RuntimeError("inside the call")
        return "plain"
    monkeypatch.setattr(Lensgroup, "_psf_lr", plain)
    orig = Lensgroup._psf_lr_grad

    def grad(self, *a, **kw):
        seen.append(("grad", self.d_sensor, kw.get("focus")))
        return orig(self, *a, **kw)
    monkeypatch.setattr(Lensgroup, "_psf_lr_grad", grad)
    return lens, seen


def test_a_number_or_a_tensor_without_grad_renders_with_that_sensor_and_puts_the_lens_back(monkeypatch):
    lens, seen = _routing_lens(monkeypatch)
    pts = torch.zeros(2, 3)
    lens.psf_lr(pts, d_sensor=62.5)
    lens.psf_lr(pts, d_sensor=torch.tensor(62.75))
    lens.psf_lr(pts, d_sensor=torch.tensor([63.0], dtype=torch.float64))
    with torch.no_grad():
        lens.psf_lr(pts, d_sensor=torch.tensor(63.25, requires_grad=True))
    lens.psf_diff(pts, d_sensor=63.5)
    lens.psf_lr(pts)
    assert seen == [("plain", 62.5), ("plain", 62.75), ("plain", 63.0), ("plain", 63.25), ("plain", 63.5),
                    ("plain", 62.25)]
    assert lens.d_sensor == 62.25 and isinstance(lens.d_sensor, float)


def test_the_lens_is_put_back_when_the_call_raises(monkeypatch):
    lens, seen = _routing_lens(monkeypatch, raises=True)
    with pytest.raises(RuntimeError):
        lens.psf_lr(torch.zeros(1, 3), d_sensor=70.0)
    assert seen == [("plain", 70.0)] and lens.d_sensor == 62.25


@pytest.mark.parametrize("kw", [dict(defer=True), dict(out=(torch.empty(1), torch.empty(1))),
                                dict(center_out=torch.empty(1, 2))])
@pytest.mark.parametrize("center", [True, False])
def test_a_sensor_that_requires_grad_takes_the_grad_path_which_refuses_defer_out_and_center_out(monkeypatch, kw, center):
    lens, seen = _routing_lens(monkeypatch)
    s = torch.tensor(62.5, requires_grad=True)
    with pytest.raises(ValueError):
        lens.psf_lr(torch.zeros(1, 3), center=center, d_sensor=s, **kw)
    assert len(seen) == 1 and seen[0][0] == "grad" and seen[0][1] == 62.5 and seen[0][2] is s
    assert lens.d_sensor == 62.25


def test_psf_needs_grad_knows_the_sensor_and_only_a_scalar_gets_a_gradient(monkeypatch):
    s = torch.tensor(62.5, requires_grad=True)
    assert optics._psf_needs_grad(None, torch.zeros(1, 3), True, s)
    assert not optics._psf_needs_grad(None, torch.zeros(1, 3), True, s.detach())
    assert not optics._psf_needs_grad(None, torch.zeros(1, 3), True)
    with torch.no_grad():
        assert not optics._psf_needs_grad(None, torch.zeros(1, 3), True, s)
    lens, seen = _routing_lens(monkeypatch)
    with pytest.raises(ValueError):
        lens.psf_lr(torch.zeros(1, 3), d_sensor=torch.tensor([62.5, 62.6], requires_grad=True))
    assert seen == [] and lens.d_sensor == 62.25


def test_the_new_entries_are_declared_and_the_abi_version_stays():
    from sdirt_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    for name in ("sdirt_forward_integral_grad_focus", "sdirt_chief_center_slope"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert len(_lib.SIGNATURES["sdirt_forward_integral_grad_focus"][1]) == len(_lib.SIGNATURES["sdirt_forward_integral_grad"][1])
    assert len(_lib.SIGNATURES["sdirt_chief_center_slope"][1]) == len(_lib.SIGNATURES["sdirt_chief_center"][1]) + 1
    assert _lib.ABI_VERSION == 4 and "#define SDIRT_ABI_VERSION 4" in header
