"""Gradients of the dual-pixel splat without a GPU: the float64 restatement (tests/splat_f64.py) against the reference's
own autograd gradients (computed afresh by tools/gen_golden_dp_grad.py where the reference checkout is present), and
the rules that decide which psf_lr calls record gradients."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_state
from splat_f64 import max_normalise, splat_f64

from sdirt_amd import optics
from sdirt_amd.optics import Lensgroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def f27():
    """The reference's cases (tools/gen_golden_dp_grad.py): small and big r, both directions, both centre rules."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_dp_grad as gen
    return gen.cases(check_repeat=False)


def _case(g, i):
    p = f"c{i}_"
    return {k[len(p):]: v for k, v in g.items() if k.startswith(p)}


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")
def test_restatement_matches_reference_float64_gradients(f27):
    ks = int(f27["ks"])
    ps = load_state("rf50mm")["pixel_size"]
    cases = [_case(f27, i) for i in range(int(f27["n_cases"]))]
    assert {float(c["dp"][3]) > 0.5 for c in cases} == {False, True}
    assert {int(c["direct"]) for c in cases} == {0, 1} and {int(c["center"]) for c in cases} == {0, 1}
    for c in cases:
        assert np.all(np.isfinite(c["grad32"])) and np.all(np.isfinite(c["grad64"]))
        rays = [torch.from_numpy(c[k]) for k in ("ox", "oy", "dx", "dz", "ra")]
        h, f, w = (torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in c["dp"][:3])
        cen = torch.tensor(c["pointc"], dtype=torch.float64, requires_grad=True)
        # the reference's float64 run tested the window in float64
        L, R = splat_f64(*rays, cen, ps, ks, h, f, w, float(c["dp"][3]), mask_dtype=torch.float64)
        psf = max_normalise(R if int(c["direct"]) else L)
        assert np.abs(psf.detach().numpy() - c["psf"]).max() < 1e-5          # the fp32 run's PSF
        (torch.from_numpy(c["G"]).double() * psf).sum().backward()
        got = np.array([float(h.grad), float(f.grad), float(w.grad)])
        np.testing.assert_allclose(got, c["grad64"], rtol=1e-9, atol=0)
        if not int(c["center"]):
            np.testing.assert_allclose(cen.grad.numpy(), c["gcen64"], rtol=1e-9, atol=1e-12)


def test_restatement_is_finite_where_the_segment_area_is_not_differentiable():
    """|x| = r inside the clamp range: the chord form gives 0 where acos' derivative is infinite."""
    h, f, w = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (0.78, 1.44, 0.5))
    x_tan = torch.zeros((1, 1), dtype=torch.float32)      # margin boundary x = w - h * 0 = 0.5 = r exactly
    one = torch.ones((1, 1), dtype=torch.float32)
    L, R = splat_f64(0 * one, 0 * one, x_tan, one, one, torch.zeros(1, 2, dtype=torch.float64), 0.01, 5, h, f, w, 0.5)
    (L.sum() + 2 * R.sum()).backward()
    assert all(torch.isfinite(t.grad) for t in (h, f, w))


# ------------------------------------------------------------------ which calls record gradients
def _routing_lens(monkeypatch):
    lens = Lensgroup.__new__(Lensgroup)
    seen = []
    monkeypatch.setattr(Lensgroup, "_psf_lr", lambda self, *a: seen.append("plain") or "plain")
    orig = Lensgroup._psf_lr_grad

    def grad(self, *a):
        seen.append("grad")
        return orig(self, *a)
    monkeypatch.setattr(Lensgroup, "_psf_lr_grad", grad)
    return lens, seen


def test_plain_floats_no_grad_and_detached_tensors_take_the_existing_path(monkeypatch):
    lens, seen = _routing_lens(monkeypatch)
    pts = torch.zeros(2, 3, requires_grad=True)
    lens.psf_lr(pts, dp=(0.78, 1.44, 0.3, 0.5))                                  # floats; points with center=True
    lens.psf_lr(torch.zeros(2, 3), dp=(torch.tensor(0.78), 1.44, 0.3, 0.5))     # tensors without grad
    lens.psf_lr(torch.zeros(2, 3), dp=(0.78, 1.44, 0.3, torch.tensor(0.5, requires_grad=True)))   # r: no gradient
    with torch.no_grad():
        lens.psf_lr(torch.zeros(2, 3), dp=(torch.tensor(0.78, requires_grad=True), 1.44, 0.3, 0.5))
        lens.psf_lr(pts, center=False)
    assert seen == ["plain"] * 5


@pytest.mark.parametrize("kw", [dict(defer=True), dict(out=(torch.empty(1), torch.empty(1))),
                                dict(center_out=torch.empty(1, 2))])
def test_grad_calls_refuse_defer_out_and_center_out(monkeypatch, kw):
    lens, seen = _routing_lens(monkeypatch)
    h = torch.tensor(0.78, requires_grad=True)
    with pytest.raises(ValueError):
        lens.psf_lr(torch.zeros(1, 3), dp=(h, 1.44, 0.3, 0.5), **kw)
    assert seen == ["grad"]


def test_uncentred_points_that_require_grad_record_gradients(monkeypatch):
    lens, seen = _routing_lens(monkeypatch)
    with pytest.raises(ValueError):
        lens.psf_lr(torch.zeros(1, 3, requires_grad=True), center=False, defer=True)
    assert seen == ["grad"]
    assert optics._psf_needs_grad(None, torch.zeros(1, 3, requires_grad=True), center=False)
    assert not optics._psf_needs_grad(None, torch.zeros(1, 3, requires_grad=True), center=True)
