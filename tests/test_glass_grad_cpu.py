"""Glass gradients (n, V of every medium) without a GPU: the C ABI declares the new entry, the glass round-trips through
Lensgroup.glass_parameters / set_glass_parameters / the lens JSON, and the float64 restatement with eta a function of the
glass (tests/glass_f64.py) agrees with central differences of its own forward and, where the reference checkout is
present, with the reference's own float64 autograd (tools/gen_glass_grad.py)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import glass_f64 as G
import trace_f64 as T
from conftest import make_lens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWNED = {"rf50mm": (6, 13), "rf35mm": (11, 22), "rf50mm_variant": (6, 13)}


def test_header_declares_the_eta_entry_and_the_library_exports_it():
    from sdirt_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdirt_dp.h")).read(), flags=re.S)
    h = _lib.lib()
    assert re.search(r"\bsdirt_trace2sensor_grad_eta\s*\(", txt)
    assert _lib.SIGNATURES["sdirt_trace2sensor_grad_eta"] == _lib.SIGNATURES["sdirt_trace2sensor_grad"]
    assert hasattr(h, "sdirt_trace2sensor_grad_eta")
    assert h.sdirt_abi_version() == 4
    old = re.search(r"int sdirt_trace2sensor_grad\((.*?)\);", txt, re.S).group(1)
    new = re.search(r"int sdirt_trace2sensor_grad_eta\((.*?)\);", txt, re.S).group(1)
    assert re.sub(r"\s+", " ", old) == re.sub(r"\s+", " ", new)          # the same argument list (comments dropped)


def _state(lens):
    return [(m.n, m.V, m.A, m.B, m.name) for s in lens.surfaces for m in (s.mat1, s.mat2)]


@pytest.mark.parametrize("name", sorted(OWNED))
def test_glass_parameters_round_trip_and_refuse_what_is_not_a_glass(name, tmp_path):
    from sdirt_amd import Lensgroup
    lens = make_lens(name, "cpu")
    K = len(lens.surfaces)
    glass, own = lens.glass_parameters(), lens.glass_owned()
    assert glass.shape == (K + 1, 2) and glass.dtype == torch.float64 and glass.device.type == "cpu"
    assert own.shape == (K + 1,) and own.dtype == torch.bool and (int(own.sum()), K + 1) == OWNED[name]
    assert glass is not lens.glass_parameters()
    for j in range(K + 1):
        m = lens.surfaces[j].mat1 if j < K else lens.surfaces[-1].mat2
        assert bool(own[j]) == (m.dispersion == "naive")
        assert float(glass[j, 0]) == m.n and float(glass[j, 1]) == (m.V if own[j] else 0.0)
    # writing the values back changes nothing and still invalidates
    digest, before = lens._table_digest(), _state(lens)
    lens._pupil_cache[True] = (1.0, 2.0)
    planner = lens.trips
    assert lens.set_glass_parameters(glass) is lens
    assert lens._table_digest() == digest and torch.equal(lens.glass_parameters(), glass)
    assert [(s[0], s[1], s[2], s[3]) for s in _state(lens)] == [(s[0], s[1], s[2], s[3]) for s in before]
    assert not lens._pupil_cache and not lens._dev and lens.trips is not planner
    # a moved owned entry reads back, in both objects of the medium, and the surface descriptors follow
    j = int(torch.nonzero(own)[0])
    moved = glass.clone()
    moved[j, 0] += 1.2345e-3
    moved[j, 1] *= 1.01
    n1_old = lens.surfaces[j].desc(0.486).n1
    lens.set_glass_parameters(moved)
    assert torch.equal(lens.glass_parameters(), moved)
    n, V = float(moved[j, 0]), float(moved[j, 1])
    want = n + (n - 1) / (V * G.C1) * (1 / 486.0 ** 2 - G.C2)
    assert lens.surfaces[j].desc(0.486).n1 == lens.surfaces[j - 1].desc(0.486).n2 != n1_old
    assert abs(lens.surfaces[j].desc(0.486).n1 - want) <= 1e-15 * want
    assert lens.surfaces[j].mat1.name == lens.surfaces[j - 1].mat2.name == f"{n!r}/{V!r}"
    # the JSON round trip gives the fitted lens back bit for bit
    path = str(tmp_path / "fitted.json")
    lens.write_lens_json(path)
    again = Lensgroup(path, sensor_res=lens.sensor_res, post_computation=False, device="cpu")
    assert torch.equal(again.glass_parameters(), moved) and torch.equal(again.glass_owned(), own)
    assert [s[:4] for s in _state(again)] == [s[:4] for s in _state(lens)]
    # every refusal leaves the lens as it is
    air = int(torch.nonzero(~own)[0])
    now = _state(lens)
    bad = []
    for row, col, v in ((j, 0, 1.0), (j, 0, float("nan")), (j, 1, 0.0), (j, 1, float("inf")), (j, 1, -3.0), (air, 0, 1.0003), (air, 1, 50.0)):
        b = moved.clone()
        b[row, col] = v
        bad.append(b)
    bad += [moved[:-1], moved[:, :1], moved.reshape(-1)]
    for b in bad:
        with pytest.raises(ValueError):
            lens.set_glass_parameters(b)
        assert _state(lens) == now
        with pytest.raises(ValueError):
            with lens._glass_borrowed(b):
                pass
        assert _state(lens) == now


def test_glass_borrowed_restores_values_and_object_identities():
    lens = make_lens("rf50mm", "cpu")
    lens._curved()
    lens._pupil_cache[True] = (1.0, 2.0)
    keep = (lens._dev, lens._pupil_cache, lens.trips, lens.__dict__["_curved_cache"])
    before, pupils = _state(lens), dict(lens._pupil_cache)
    glass = lens.glass_parameters()
    moved = glass.clone()
    moved[1, 0] += 2e-3
    moved[4, 1] -= 0.5

    def same():
        return (_state(lens) == before and lens._dev is keep[0] and lens._pupil_cache is keep[1] and lens.trips is keep[2]
                and lens.__dict__["_curved_cache"] is keep[3] and lens._pupil_cache == pupils)
    with lens._glass_borrowed(moved):
        assert torch.equal(lens.glass_parameters(), moved)
        assert lens._dev is not keep[0] and lens._pupil_cache is not keep[1] and lens.trips is not keep[2]
    assert same()
    with pytest.raises(RuntimeError, match="inside"):
        with lens._glass_borrowed(moved.clone().requires_grad_()):
            assert torch.equal(lens.glass_parameters(), moved)
            raise RuntimeError("inside")
    assert same()
    with lens._glass_borrowed(glass):              # the lens's own values: nothing is touched
        assert lens._dev is keep[0] and lens.trips is keep[2]
    assert same()


def test_psf_calls_take_glass_params():
    from sdirt_amd import Lensgroup
    for name in ("psf_lr", "psf_diff", "psf_rgb", "psf_volume"):
        assert "glass_params" in inspect.signature(getattr(Lensgroup, name)).parameters, name


def test_package_eta_is_the_device_table_ratio_and_the_restatement_s():
    """Lensgroup._glass_eta (what autograd differentiates) gives the n1 / n2 the device table is built from, bit for bit,
    and agrees with glass_f64.eta, which writes the Cauchy formula out on its own."""
    for name in ("rf50mm", "rf35mm"):
        lens = make_lens(name, "cpu")
        glass = lens.glass_parameters()
        glass[lens.glass_owned()] *= torch.tensor([1.0007, 0.993])
        lens.set_glass_parameters(glass)
        for wv in (0.486, 0.589, 0.656):
            e = lens._glass_eta(glass, wv)
            assert e.dtype == torch.float64
            assert e.tolist() == [s.desc(wv).n1 / s.desc(wv).n2 for s in lens.surfaces]
            np.testing.assert_allclose(G.eta(glass, lens, wv).numpy(), e.numpy(), rtol=1e-14, atol=0)


def _bundle(lens, M, g):
    first = lens.surfaces[0]
    o = torch.tensor([[100.0, 50.0, -1500.0]], dtype=torch.float64).expand(M, 3)
    rad = torch.rand(M, generator=g).double().sqrt() * first.r * 0.5
    ang = torch.rand(M, generator=g).double() * 2 * np.pi
    aim = torch.stack((rad * ang.cos(), rad * ang.sin(), torch.full((M,), float(first.d), dtype=torch.float64)), -1)
    return o, torch.nn.functional.normalize(aim - o, dim=-1)


@pytest.mark.parametrize("name", ["rf50mm", "rf35mm"])
def test_restatement_glass_gradient_matches_central_differences_of_its_own_forward(name):
    """Steps 1e-6 in n and 1e-3 in V, bound 1e-4 |fd| + 1e-6, 64 rays, at 0.486 and 0.656; at 0.486 V of every owned medium
    has a gradient; at 0.5893 dn(lambda)/dV vanishes identically."""
    lens = make_lens(name, "cpu")
    K = len(lens.surfaces)
    theta, glass, own = lens.surface_parameters().double(), lens.glass_parameters(), lens.glass_owned()
    g = torch.Generator().manual_seed(1)
    M = 64
    o, d = _bundle(lens, M, g)
    wgt = torch.randn(M, 3, generator=g).double()

    def loss(gl, wv):
        e = G.eta(gl, lens, wv)
        so, sd = G.trace_f64(o, d, theta, G.glass_table(lens, wv, list(e)), [5] * K, lens.d_sensor)
        assert bool(torch.isfinite(so).all())
        return (so * wgt).sum() + (sd * wgt.flip(0)).sum()
    grads = {}
    for wv in (0.486, 0.656):
        gl = glass.clone().requires_grad_()
        loss(gl, wv).backward()
        grads[wv] = gl.grad
        assert bool((gl.grad[~own] == 0).all())
        for j in torch.nonzero(own).reshape(-1).tolist():
            for c, step in ((0, 1e-6), (1, 1e-3)):
                lo, hi = glass.clone(), glass.clone()
                lo[j, c] -= step
                hi[j, c] += step
                with torch.no_grad():
                    fd = float(loss(hi, wv) - loss(lo, wv)) / (2 * step)
                assert abs(fd - float(gl.grad[j, c])) <= 1e-4 * abs(fd) + 1e-6, (wv, j, c, fd, float(gl.grad[j, c]))
    assert bool((grads[0.486][own][:, 1] != 0).all()) and bool((grads[0.486][own][:, 0] != 0).all())
    # at the d line n(lambda) = n whatever V is
    gl = glass.clone().requires_grad_()
    loss(gl, 0.5893).backward()
    assert bool((gl.grad[own][:, 0] != 0).all())
    assert float(gl.grad[:, 1].abs().max()) <= 1e-12 * float(grads[0.486][:, 1].abs().max())
    # (1 / lambda_nm^2 - c2 is a few ulp of c2 there, 0.5893 * 1e3 not being 589.3 to the bit, against 1.3e-6 at 0.486)
    jac = [torch.autograd.functional.jacobian(lambda x: G.eta(x, lens, w), glass)[..., 1].abs().max() for w in (0.5893, 0.486)]
    assert float(jac[0]) <= 1e-14 * float(jac[1])
    # per-ray eta leaves give the same total through the Jacobian of eta in the glass
    wv = 0.486
    e0 = G.eta(glass, lens, wv)
    leaves = [e0[k].expand(M, 1).clone().requires_grad_() for k in range(K)]
    so, sd = G.trace_f64(o, d, theta, G.glass_table(lens, wv, leaves), [5] * K, lens.d_sensor)
    ((so * wgt).sum() + (sd * wgt.flip(0)).sum()).backward()
    ge = torch.stack([l.grad.sum() if l.grad is not None else torch.zeros((), dtype=torch.float64) for l in leaves])
    J = torch.autograd.functional.jacobian(lambda x: G.eta(x, lens, wv), glass)
    np.testing.assert_allclose(torch.einsum("k,kjc->jc", ge, J).numpy(), grads[wv].numpy(), rtol=1e-9, atol=1e-12)


def test_restatement_traces_a_refracting_plane_with_tensor_eta(tmp_path):
    """glass_f64's own plane branch: a cover glass (two refracting planes) traces as trace_f64 traces it with float etas,
    and its glass has a gradient that matches central differences."""
    lens = G.cover_glass_lens(tmp_path, "cpu")
    K = len(lens.surfaces)
    assert [s.kind for s in lens.surfaces[-2:]] == [T.PLANE, T.PLANE] and bool(lens.glass_owned()[K - 1])
    theta, glass = lens.surface_parameters().double(), lens.glass_parameters()
    o, d = _bundle(lens, 32, torch.Generator().manual_seed(2))
    so0, sd0 = T.trace_f64(o, d, theta, T.lens_table(lens, 0.486), [5] * K, lens.d_sensor)

    def sensor(gl):
        return G.trace_f64(o, d, theta, G.glass_table(lens, 0.486, list(G.eta(gl, lens, 0.486))), [5] * K, lens.d_sensor)
    so, sd = sensor(glass)
    np.testing.assert_allclose(so.numpy(), so0.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(sd.numpy(), sd0.numpy(), rtol=1e-13, atol=1e-13)
    gl = glass.clone().requires_grad_()
    sensor(gl)[0][:, 0].sum().backward()
    lo, hi = glass.clone(), glass.clone()
    lo[K - 1, 0] -= 1e-6
    hi[K - 1, 0] += 1e-6
    fd = float(sensor(hi)[0][:, 0].sum() - sensor(lo)[0][:, 0].sum()) / 2e-6
    assert fd != 0 and abs(fd - float(gl.grad[K - 1, 0])) <= 1e-4 * abs(fd) + 1e-6


needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_glass_grad as gen
    return gen


def _assert_owned_gradients_match(lens, case, grad):
    own = lens.glass_owned().numpy()
    assert own.sum() > 0 and np.abs(case["grad64"][own][:, 0]).min() > 0
    # (atol: an entry that vanishes by symmetry is rounding noise on both sides)
    np.testing.assert_allclose(grad.numpy()[own], case["grad64"][own], rtol=1e-9, atol=1e-12 * np.abs(case["grad64"]).max())
    assert bool((grad.numpy()[~own] == 0).all()) and bool((case["grad64"][~own] == 0).all())


@needs_reference
def test_restatement_matches_reference_float64_glass_gradients():
    """Field corners at 0.3 m and 20 m, both lenses, at 0.486, 0.589 and 0.656 um."""
    cases = _generator().cases()
    assert {(c["lens"], c["wvln"]) for c in cases} == {(n, w) for n in ("rf50mm", "rf35mm") for w in (0.486, 0.589, 0.656)}
    for case in cases:
        lens = make_lens(case["lens"], "cpu")
        glass = lens.glass_parameters().requires_grad_()
        table = G.glass_table(lens, case["wvln"], list(G.eta(glass, lens, case["wvln"])))
        so, sd = G.trace_f64(torch.from_numpy(case["o"]), torch.from_numpy(case["d"]), lens.surface_parameters().double(), table,
                             case["trips"], case["d_sensor"])
        ((so * torch.from_numpy(case["wo"])).sum() + (sd * torch.from_numpy(case["wd"])).sum()).backward()
        _assert_owned_gradients_match(lens, case, glass.grad)


@needs_reference
def test_psf_restatement_matches_reference_float64_glass_gradients():
    """The trace chained with splat_f64 against the reference's trace2sensor + forward_integral graph in float64: both
    centre rules, both area models, both directions, near and far, both lenses, at 0.486 and 0.656 um."""
    cases = _generator().psf_cases()
    assert {c["wvln"] for c in cases} == {0.486, 0.656} and {c["lens"] for c in cases} == {"rf50mm", "rf35mm"}
    for case in cases:
        lens = make_lens(case["lens"], "cpu")
        glass = lens.glass_parameters().requires_grad_()
        table = G.glass_table(lens, case["wvln"], list(G.eta(glass, lens, case["wvln"])))
        h, f, w = (torch.tensor(v, dtype=torch.float64) for v in case["dp"][:3])
        so, sd = G.trace_f64(torch.from_numpy(case["o"]), torch.from_numpy(case["d"]), lens.surface_parameters().double(), table,
                             case["trips"], case["d_sensor"])
        from splat_f64 import splat_f64
        S = len(case["o"])
        sn = lambda v: v.reshape(1, S).t()
        L, R = splat_f64(sn(so[:, 0]), sn(so[:, 1]), sn(sd[:, 0]), sn(sd[:, 2]), torch.ones(S, 1, dtype=torch.float32),
                         torch.from_numpy(case["center"]), case["ps"], case["ks"], h, f, w, float(case["dp"][3]), mask_dtype=torch.float64)
        (torch.from_numpy(case["G"]) * (R if case["direct"] == "r" else L)).sum().backward()
        _assert_owned_gradients_match(lens, case, glass.grad)
