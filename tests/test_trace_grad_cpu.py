"""Surface-parameter gradients without a GPU: the C ABI declares the new entries, the prescription round-trips through
Lensgroup.surface_parameters / set_surface_parameters, and the float64 restatement of the trace (tests/trace_f64.py)
agrees with central differences of its own forward and, where the reference checkout is present, with the reference's
own float64 autograd (tools/gen_trace_grad.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import trace_f64 as T
from conftest import make_lens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sdirt_forward_integral_grad_rays", "sdirt_trace2sensor_grad_workspace_bytes", "sdirt_trace2sensor_record",
               "sdirt_trace2sensor_grad_workgroups", "sdirt_trace2sensor_grad")


def test_header_declares_the_new_entries_and_the_library_exports_them():
    from sdirt_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdirt_dp.h")).read(), flags=re.S)
    h = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.sdirt_trace2sensor_grad_workspace_bytes(1000, 12) == 24 * 13 * 1000
    assert h.sdirt_trace2sensor_grad_workgroups(1 << 24, 256) == 8 * 256
    assert h.sdirt_trace2sensor_grad_workgroups(300, 256) == 2
    assert h.sdirt_abi_version() == 4


@pytest.mark.parametrize("name", ["rf50mm", "rf35mm"])
def test_surface_parameters_round_trip_and_refuse_foreign_columns(name):
    from sdirt_amd import _lib
    lens = make_lens(name, "cpu")
    K = len(lens.surfaces)
    theta = lens.surface_parameters()
    assert theta.shape == (K, 3 + _lib.MAX_AI) and theta.dtype == torch.float32
    for k, s in enumerate(lens.surfaces):
        assert float(theta[k, 0]) == float(s.d) and float(theta[k, 1]) == float(s.c) and float(theta[k, 2]) == float(s.k)
        deg = s.ai_degree if s.ai is not None else 0
        assert np.array_equal(theta[k, 3:3 + deg].numpy(), s.ai if deg else np.zeros(0, np.float32))
        assert bool((theta[k, 3 + deg:] == 0).all())
    digest = lens._table_digest()
    lens._pupil_cache[True] = (1.0, 2.0)
    planner = lens.trips
    lens.set_surface_parameters(theta)
    assert lens._table_digest() == digest and torch.equal(lens.surface_parameters(), theta)
    assert not lens._pupil_cache and not lens._dev and lens.trips is not planner       # invalidated all the same
    # every owned entry can be written and read back
    own = torch.from_numpy(np.stack([s.owned_columns() for s in lens.surfaces]))
    kinds = [s.kind for s in lens.surfaces]
    moved = torch.where(own, theta * 1.001 + 1e-4 * (theta == 0), theta)
    lens.set_surface_parameters(moved)
    assert torch.equal(lens.surface_parameters(), moved) and [s.kind for s in lens.surfaces] == kinds
    assert theta is not lens.surface_parameters() and not torch.equal(theta, moved)
    # the stop owns d alone; a sphere's k and a curvature of 0 would change the surface's kind
    stop = lens.aper_idx
    sphere = kinds.index(_lib.KIND_SPHERE)
    for k, c, v in ((stop, 1, 0.01), (sphere, 2, -0.5), (sphere, 1, 0.0), (sphere, 3, 1e-6)):
        bad = moved.clone()
        bad[k, c] = v
        with pytest.raises(ValueError):
            lens.set_surface_parameters(bad)
        assert torch.equal(lens.surface_parameters(), moved)
    with pytest.raises(ValueError):
        lens.set_surface_parameters(moved[:-1])


@pytest.mark.parametrize("name, conic", [("rf50mm", None), ("rf35mm", None), ("rf50mm", T.CONIC["rf50mm"]), ("rf35mm", T.CONIC["rf35mm"])])
def test_restatement_gradients_match_central_differences_of_its_own_forward(name, conic):
    lens = T.with_conic(make_lens(name, "cpu"), conic)
    assert all(lens.surfaces[i].owned_columns()[2] for i in (conic or {}))
    K = len(lens.surfaces)
    theta = lens.surface_parameters().double()
    table = T.lens_table(lens, 0.589)
    g = torch.Generator().manual_seed(1)
    M, first = 64, lens.surfaces[0]
    o = torch.tensor([[100.0, 50.0, -1500.0]], dtype=torch.float64).expand(M, 3)
    rad = torch.rand(M, generator=g).double().sqrt() * first.r * 0.5
    ang = torch.rand(M, generator=g).double() * 2 * np.pi
    aim = torch.stack((rad * ang.cos(), rad * ang.sin(), torch.full((M,), float(first.d), dtype=torch.float64)), -1)
    d = torch.nn.functional.normalize(aim - o, dim=-1)
    wgt = torch.randn(M, 3, generator=g).double()

    def loss(th):
        so, sd = T.trace_f64(o, d, th, table, [5] * K, lens.d_sensor)
        assert bool(torch.isfinite(so).all())
        return (so * wgt).sum() + (sd * wgt.flip(0)).sum()
    th = theta.clone().requires_grad_()
    loss(th).backward()
    own = np.stack([s.owned_columns() for s in lens.surfaces])
    for k, c in np.argwhere(own):
        # d, c, k: an absolute step of 1e-6; ai_j multiplies r2^(j+1) with r2 ~ 100 mm^2: a step that moves the sag alike
        step = 1e-6 * max(1.0, abs(float(theta[k, c]))) if c < 3 else max(1e-3 * abs(float(theta[k, c])), 1e-6 / 100.0 ** (c - 2))
        lo, hi = theta.clone(), theta.clone()
        lo[k, c] -= step
        hi[k, c] += step
        fd = float(loss(hi) - loss(lo)) / (2 * step)
        assert abs(fd - float(th.grad[k, c])) <= 1e-4 * abs(fd) + 1e-6, (k, c, fd, float(th.grad[k, c]))
    # per-ray leaves give the same total
    pr = theta.unsqueeze(0).expand(M, -1, -1).clone().requires_grad_()
    loss(pr).backward()
    np.testing.assert_allclose(pr.grad.sum(0).numpy(), th.grad.numpy(), rtol=1e-10, atol=1e-12)


needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_trace_grad as gen
    return gen


def _assert_owned_gradients_match(lens, case, grad):
    own = np.stack([s.owned_columns() for s in lens.surfaces])
    for i in (case["conic"] or {}):
        assert own[i, 2], "a conic constant != 0 is a parameter of its asphere"
    # (atol: an entry that vanishes by symmetry is rounding noise on both sides)
    np.testing.assert_allclose(grad.numpy()[own], case["grad64"][own], rtol=1e-9, atol=1e-12 * np.abs(case["grad64"]).max())
    return own


@needs_reference
def test_restatement_matches_reference_float64_gradients():
    """Field corners at 0.3 m and 20 m, both lenses, and the aspheres with k != 0 (above and below -1)."""
    cases = _generator().cases()
    assert any(c["conic"] for c in cases)
    for case in cases:
        lens = T.with_conic(make_lens(case["lens"], "cpu"), case["conic"])
        theta = lens.surface_parameters().double().requires_grad_()
        so, sd = T.trace_f64(torch.from_numpy(case["o"]), torch.from_numpy(case["d"]), theta, T.lens_table(lens, case["wvln"]),
                             case["trips"], case["d_sensor"])
        ((so * torch.from_numpy(case["wo"])).sum() + (sd * torch.from_numpy(case["wd"])).sum()).backward()
        own = _assert_owned_gradients_match(lens, case, theta.grad)
        for i in (case["conic"] or {}):
            assert case["grad64"][i, 2] != 0


@needs_reference
def test_psf_restatement_matches_reference_float64_gradients():
    """The trace chained with splat_f64 against the reference's trace2sensor + forward_integral graph in float64: both
    centre rules, both area models, both directions, a field corner at 0.3 m and at 20 m, both lenses."""
    cases = _generator().psf_cases()
    assert {(c["lens"], float(c["o"][0, 2]) > -1000, c["dp"][3] > 0.5) for c in cases} >= {
        (n, near, big) for n in ("rf50mm", "rf35mm") for near in (True, False) for big in (True, False)}
    for case in cases:
        lens = T.with_conic(make_lens(case["lens"], "cpu"), case["conic"])
        theta = lens.surface_parameters().double().requires_grad_()
        h, f, w = (torch.tensor(v, dtype=torch.float64) for v in case["dp"][:3])
        L, R = T.psf_f64(torch.from_numpy(case["o"]), torch.from_numpy(case["d"]), theta, T.lens_table(lens, case["wvln"]),
                         case["trips"], case["d_sensor"], len(case["o"]), 1, torch.from_numpy(case["center"]), case["ps"],
                         case["ks"], (h, f, w, case["dp"][3]), mask_dtype=torch.float64)
        (torch.from_numpy(case["G"]) * (R if case["direct"] == "r" else L)).sum().backward()
        _assert_owned_gradients_match(lens, case, theta.grad)
