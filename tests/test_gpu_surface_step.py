"""One surface visit (sdirt_device.hpp: sag_g_dgd, newton_k, refract, curved_reaction, surface_reaction) on the
prescriptions the random fuzz of test_gpu_properties.py never draws.

The per-ray arithmetic of a visit is shared by every kernel that traces, and its wave-uniform decisions -- the
polynomial's degree, the kind of the surface, the sign of its curvature, the direction of travel, 1 + k == 1 -- are
branches and scalar selects around that arithmetic: a wrong one is a wrong term or a wrong sign, not a small error.
So everything here is bit equality.

  staged trace        k_trace, forward and backward, both math policies, against the CPU oracle: positions, directions,
                      weights, obliquity and the Newton trip tables.  Hand-built prescriptions: even aspheres of degree
                      1, 2, 3, 4, 7 and 8 (the fuzz is always degree 6; its coefficient scales, extended by 1e-15 and
                      1e-17), k == 0 with polynomial terms, k <= -1 with terms, pure conics (k > -1, k <= -1 and k == 0:
                      the unit-k Newton copy on a surface that is no sphere), spheres and aspheres of both curvature signs
                      on either side of a glass, a refracting plane.  64 rays of every bundle lie exactly on the axis and
                      64 have dx == 0 (half of them x == 0 as well: the normal's x component is a zero all the way), where
                      the sign of a zero is all that a negated normal leaves behind.
  fused / two-stage   sdirt_psf_lr_centered (chief-ray pass inside k_psf_lr) against sdirt_chief_center followed by
                      sdirt_psf_lr (k_chief_center, then the kernels without the chief-ray pass) on one of those
                      prescriptions and on rf35mm: chief-ray centres, both convergence-mask rows and the ks 21 PSFs
                      (float64 tiles: sums do not depend on their order).

Every case traces 4096 rays, or 5 points x (700 + 2048) rays."""
import json

import numpy as np
import pytest
import torch

from conftest import load_state, make_lens

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = ["1.51680/64.2", "1.80518/25.4", "1.67270/32.1", "1.53110/55.9"]
AI_SCALES = (2e-4, 2e-5, 2e-7, 1e-9, 1e-11, 1e-13, 1e-15, 1e-17)


def _ai(seed, degree):
    rng = np.random.default_rng(seed)
    return [float(rng.normal(0, s)) for s in AI_SCALES[:degree]]


def _build(rows, d_sensor_behind=30.0):
    """rows: (kind, semi-aperture, curvature, glass before, glass after, conic, ai or None, distance to the next vertex)
    -> (the package's own JSON schema, the per-surface state the oracle helpers read)."""
    from sdirt_amd.basics import Material
    surfaces, z = [], 0.0
    for kind, semi, c, ga, gb, k, ai, gap in rows:
        s = dict(kind=kind, semi_aperture=semi, z=z, curvature=c, glass_before=ga, glass_after=gb)
        if kind == "asphere":
            s["conic"], s["even_asphere"] = k, list(ai)
        surfaces.append(s)
        z += gap
    data = dict(name="surface_step", units="mm", r_last=21.64, d_sensor=z + d_sensor_behind, sensor_size=[24.0, 36.0],
                surfaces=surfaces)
    key = repr(0.589)
    state = dict(surfaces=[dict(
        kind=s["kind"], r=s["semi_aperture"], d=s["z"], c=s["curvature"], k=s.get("conic", 0.0),
        ai=s.get("even_asphere", []) if s["kind"] == "asphere" else [],
        n1={key: float(Material(s["glass_before"]).ior(0.589))},
        n2={key: float(Material(s["glass_after"]).ior(0.589))}) for s in surfaces])
    return data, state


def _window(glass):
    return [("plane", 9.0, 0.0, "air", glass, 0.0, None, 1.0), ("plane", 9.0, 0.0, glass, "air", 0.0, None, 1.0)]


STOP = ("plane", 5.0, 0.0, "air", "air", 0.0, None, 2.0)
PRESCRIPTIONS = {
    # degrees 1 - 4; k == 0 with terms, k < -1 with terms, k == -1 with terms; an asphere of either curvature sign on
    # either side of a glass; a refracting plane
    "degrees_1_to_4": [
        ("asphere", 9.0, 0.035, "air", G[0], 0.0, _ai(1, 1), 3.0),
        ("asphere", 9.0, -0.020, G[0], "air", -1.5, _ai(2, 2), 2.0),
        STOP,
        ("asphere", 9.0, -0.030, "air", G[1], 0.4, _ai(3, 3), 2.5),
        ("asphere", 9.0, 0.015, G[1], "air", -1.0, _ai(4, 4), 2.0),
    ] + _window(G[0]),
    # degrees 7 and 8 (r2 ** 8 in fp64), beside spheres that meet the glass with the other two sign combinations
    "degrees_7_and_8": [
        ("sphere", 9.0, -0.020, "air", G[2], 0.0, None, 3.0),
        ("asphere", 9.0, -0.050, G[2], "air", 0.0, _ai(7, 7), 2.0),
        STOP,
        ("asphere", 9.0, 0.040, "air", G[3], -2.2, _ai(8, 8), 3.5),
        ("sphere", 9.0, 0.012, G[3], "air", 0.0, None, 2.0),
    ],
    # pure conics on both sides of k = -1 and at k == 0 (no sphere, but 1 + k == 1), spheres entering with c > 0 and
    # leaving with c < 0, degree 6 with k == 0, a refracting plane
    "conics_and_spheres": [
        ("sphere", 9.0, 0.030, "air", G[1], 0.0, None, 3.0),
        ("sphere", 9.0, -0.025, G[1], "air", 0.0, None, 2.0),
        STOP,
        ("asphere", 9.0, 0.030, "air", G[0], -0.6, [], 2.5),
        ("asphere", 9.0, -0.020, G[0], "air", -1.8, [], 1.5),
        ("asphere", 9.0, 0.020, "air", G[3], 0.0, [], 2.5),
        ("asphere", 9.0, -0.030, G[3], "air", 0.0, _ai(6, 6), 2.0),
    ] + _window(G[2]),
}


def _bundle(rng, n, backward, d_sensor):
    """The fuzz's bundle, with 64 rays exactly on the axis and 64 with dx == 0 (32 of them with x == 0 too)."""
    o = np.zeros((n, 3), np.float32)
    o[:, :2] = rng.uniform(-6, 6, (n, 2))
    o[:, 2] = d_sensor if backward else -50.0
    d = np.zeros((n, 3), np.float64)
    d[:, :2] = rng.normal(0, 0.08, (n, 2))
    d[:, 2] = -1.0 if backward else 1.0
    o[:64, :2] = 0.0
    d[:64, :2] = 0.0
    d[64:128, 0] = 0.0
    o[64:96, 0] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    assert np.all(d[:128, 0] == 0.0) and np.all(np.abs(d[:64, 2]) == 1.0)
    return o, d


@pytest.fixture(scope="module")
def traced(oracle):
    """name -> (prescription, {backward: (o, d, the oracle's trace)}): computed once, shared, left unchanged."""
    out = {}
    for i, (name, rows) in enumerate(PRESCRIPTIONS.items()):
        data, state = _build(rows)
        surf = oracle.surfaces_from_state(state, 0.589)
        rng = np.random.default_rng(50 + i)
        runs = {}
        for backward in (False, True):
            o, d = _bundle(rng, 4096, backward, data["d_sensor"])
            runs[backward] = (o, d, oracle.trace(surf, o, d, np.ones(len(o), np.float32)))
        out[name] = (data, runs)
    return out


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("name", sorted(PRESCRIPTIONS))
def test_hand_built_prescriptions_trace_bit_exact_against_the_oracle(traced, tmp_path, name, backward, precision):
    from sdirt_amd import Lensgroup
    from test_gpu_parity import rays_from_fixture
    data, runs = traced[name]
    o, d, ref = runs[backward]
    assert 0.02 < ref["ra"].mean() <= 1.0, "degenerate prescription: no case may pass on dead rays"
    assert ref["ra"][:64].all(), "the on-axis rays must get through"
    path = tmp_path / "surface_step.json"
    path.write_text(json.dumps(data))
    K = len(data["surfaces"])
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    lens.precision = precision
    ray, valid, _ = lens.trace(rays_from_fixture(o, d))
    key = ("trace", 0.589, 0, K, not backward, precision)
    assert np.array_equal(lens.trips.cache[key], ref["trips"]), (name, backward, precision)
    assert np.array_equal(ray.ra.cpu().numpy(), ref["ra"])
    # bit patterns: the sign of a zero counts (array_equal alone takes -0 for +0)
    for what, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got, ref[what]), (what, name, backward, precision)
        live = ref["ra"] > 0
        assert np.array_equal(got[live].view(np.int32), np.ascontiguousarray(ref[what][live]).view(np.int32)), \
            (what, "bit patterns of the live rays", name, backward, precision)


# ---- fused against the two-stage launches ---------------------------------------------------------------------------
SPP = 700


def _setup_rf35():
    from test_gpu_psf_kernarg_blocks import POINTS, Setup
    return Setup(make_lens("rf35mm", DEV, load_state("rf35mm")), POINTS, SPP)


def _setup_hand_built(tmp_path):
    """`degrees_1_to_4` with hand-chosen object points and aim discs on its first vertex plane (the prescription has no
    fitted pupil), and a pixel wide enough for its unfocused spots: a 21 x 0.25 mm window."""
    from sdirt_amd import Lensgroup
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import SC, Setup, _disc
    data, _ = _build(PRESCRIPTIONS["degrees_1_to_4"])
    path = tmp_path / "surface_step_psf.json"
    path.write_text(json.dumps(data))
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    s = object.__new__(Setup)
    s.lens, s.S, s.W = lens, SPP, 1
    s.po = torch.tensor([[0.0, 0.0, -1500.0], [40.0, -30.0, -1200.0], [-25.0, 35.0, -2500.0], [5.0, 5.0, -600.0],
                         [0.0, 60.0, -3000.0]], device=DEV)
    s.N = s.po.shape[0]
    s.x2, s.y2 = (v[None].contiguous() for v in _disc(SPP, 4.0, 3))
    s.xc, s.yc = (v[None].contiguous() for v in _disc(SC, 1.0, 8))
    s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
    s.st = stream_ptr(lens.device)
    return s


@pytest.mark.parametrize("which", ["hand_built", "rf35mm"])
def test_fused_against_two_stage_centres_masks_and_psfs(tmp_path, which):
    from sdirt_amd import _lib
    from test_gpu_psf_kernarg_blocks import _assert_same, fused, unfused
    s = _setup_hand_built(tmp_path) if which == "hand_built" else _setup_rf35()
    n_cus = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    assert _lib.lib().sdirt_psf_spp_slices(s.N, SPP, n_cus) == 1          # fused: the CENTER instantiations
    for f in (_lib.PSF_NORMALIZE, 0, _lib.PSF_STRICT_IEEE):
        _assert_same(fused(s, 21, f), unfused(s, 21, f), f"{which}, flags {f}")
