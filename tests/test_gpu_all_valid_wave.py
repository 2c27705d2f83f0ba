"""Waves whose 64 rays all pass a validity test beside waves with exactly one ray that fails it (sdirt_device.hpp:
zero_outside_wave in newton_k -- the Lean fused kernels branch over `inside ? rr : 0` when the compare's lane mask
equals exec, and run the select in place otherwise).  A select whose mask is all ones is its true operand, so nothing
here states new behaviour: every check is bit equality against the CPU oracle (staged trace) or between the fused
kernel and the two-stage launches, and the file passes on a library without the fast path as well.

  bundles     128 rays = two waves.  Nine per case, traced in one launch (1152 rays, every bundle on a wave boundary):
              both waves all valid; wave 0 all valid and wave 1 with ONE failing ray in lane 0, 31, 32 or 63; the
              mirror image of each (the failing ray in wave 0).
  the failing ray, one case each
    tail      outside lim_tight (the aperture) at the Newton tail -- sphere, conic k = 1, conic k = -3, asphere with
              four terms, one surface each.
    stop      stopped by an aperture plane one surface earlier, so that it ENTERS the curved surface dead -- the same
              four kinds behind a stop, and a three-surface lens (stop, sphere, conic) whose last two visits it enters
              dead.
    grazing   c2i <= 0.1 at Snell: a sphere of semi-aperture 0.96 R met at 0.955 R from air.
    tir       total internal reflection at Snell: a sphere met at 0.72 R from the glass side.
    nan       a NaN t: a direction with dz == 0 -- sphere, asphere with terms.
    leaves    leaves lim_loose in a Newton trip behind the first one, so that its wave runs the select in some trips
              and the fast path in the others.  A ray that is outside in ONE trip and converged afterwards would
              test the select alone, but does not exist on a conic: outside the domain the sag is evaluated at
              r2 = 0, the step goes back to the vertex plane, and the ray walks out again;
              test_no_ray_leaves_the_domain_and_converges is the float64 search (2 * 10^5 rays, none).  So this ray
              is dead at the end, as the oracle says.
  the cap     every pool is filled from candidates that the oracle itself (record=True) has sorted: alive to the end,
              or dead from the surface and by the half of the visit (position committed or not) the case is about;
              and the assembled launch is traced by the oracle first, which must kill EXACTLY the nine failing rays --
              asserted before anything runs on the GPU.
  checks      forward and backward, Lean and strict IEEE: the staged trace against the oracle, bit for bit in position,
              direction, obliquity, weight and the trip table (the convergence masks of the trips that ran).
              The fused kernel against sdirt_chief_center + sdirt_psf_lr on the forward lenses: 2 points, 64, 65 and
              128 samples aimed at the bundles, 64 chief rays -- centres, L, R and both mask rows.

Lean::div by zero is NaN where the reference has inf (sdirt_device.hpp); a ray with dz == 0 is dead under both and a
dead ray keeps its state, which is what is compared."""
import json

import numpy as np
import pytest
import torch

from test_gpu_surface_step import G, _ai, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CURV = 2.0 ** -4
RADIUS = 1.0 / CURV
LANES = (0, 31, 32, 63)
KINDS = {"sphere": ("sphere", 0.0, None), "conic_k1": ("asphere", 1.0, []), "conic_km3": ("asphere", -3.0, []),
         "asphere_terms": ("asphere", 0.0, _ai(43, 4))}
CASES = [("tail", k) for k in sorted(KINDS)] + [("stop", k) for k in sorted(KINDS)] + [
    ("stop", "three_surfaces"), ("grazing", "sphere"), ("tir", "sphere"), ("nan", "sphere"), ("nan", "asphere_terms"),
    ("leaves", "sphere")]
GAP = 3.0


def _curved(kind, semi, backward, exits=False, c=CURV, glass=G[0]):
    """One curved surface that the ray, in ITS direction of travel, enters from air (exits: from the glass)."""
    ref_kind, k, ai = KINDS[kind]
    first, second = (glass, "air") if exits else ("air", glass)
    before, after = (second, first) if backward else (first, second)
    return (ref_kind, semi, c, before, after, k, ai, GAP)


def _stop(r):
    return ("plane", r, 0.0, "air", "air", 0.0, None, GAP)


def _lens_rows(case, kind, backward):
    """The prescription in z order; the rows are written in the order the ray meets them."""
    if case in ("tail", "nan"):
        met = [_curved(kind, 4.0, backward)]
    elif case == "stop" and kind == "three_surfaces":
        met = [_stop(3.0), _curved("sphere", 6.0, backward), _curved("conic_k1", 6.0, backward, exits=True, c=-CURV)]
    elif case == "stop":
        met = [_stop(3.0), _curved(kind, 6.0, backward)]
    elif case == "grazing":
        met = [_curved(kind, 0.96 * RADIUS, backward)]
    elif case == "tir":
        met = [_curved(kind, 0.96 * RADIUS, backward, exits=True)]
    else:
        met = [_curved(kind, 0.96 * RADIUS, backward)]
    return met[::-1] if backward else met


def _parallel(rng, n, h_lo, h_hi, z0, backward):
    h, th = rng.uniform(h_lo, h_hi, n), rng.uniform(0, 2 * np.pi, n)
    o = np.stack([h * np.cos(th), h * np.sin(th), np.full(n, z0)], axis=1).astype(F32)
    d = np.zeros_like(o)
    d[:, 2] = -1.0 if backward else 1.0
    return o, d


def newton_outside_trips(c, k, vertex, lim_loose, o, d, trips=10):
    """surfaces.py:523-567 restated in float64 for a conic without terms -> (how many trips evaluate outside lim_loose,
    whether the first one does, the smallest relative distance of a trip's rr from lim_loose, the last |ft| -- inf for a
    ray that ends outside)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        t = (vertex - o[:, 2]) / d[:, 2]
        dd = d[:, 0] ** 2 + d[:, 1] ** 2
        dox = d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1]
        n_out, first_out, margin = np.zeros(len(o), int), np.zeros(len(o), bool), np.full(len(o), np.inf)
        for j in range(trips):
            x, y, z = (o[:, i] + d[:, i] * t for i in range(3))
            rr = x * x + y * y
            out = ~(rr < lim_loose)
            n_out += out
            if j == 0:
                first_out = out
            margin = np.minimum(margin, np.abs(rr - lim_loose) / lim_loose)
            r2 = np.where(out, 0.0, rr)
            a = (1 + k) * r2 * c * c
            sf = np.sqrt(1 - a)
            g = r2 * c / (1 + sf)
            dgd = (1 + sf + 0.5 * a / sf) * c / (1 + sf) ** 2
            ft = g + vertex - z
            t = t - np.clip(ft / (dgd * 2 * (dd * t + dox) - d[:, 2] + 1e-9), -5, 5)
        ends_inside = (o[:, 0] + d[:, 0] * t) ** 2 + (o[:, 1] + d[:, 1] * t) ** 2 < lim_loose
    # (a ray that is outside in EVERY trip sits on the vertex plane with ft == 0: it ends outside)
    return n_out, first_out, margin, np.where(ends_inside, np.abs(ft), np.inf)


def _tilted(rng, n, z0, backward):
    o = np.zeros((n, 3))
    o[:, 0], o[:, 1], o[:, 2] = rng.uniform(-1.5, 1.5, n) * RADIUS, rng.uniform(-0.3, 0.3, n), z0
    d = np.zeros((n, 3))
    d[:, 0], d[:, 1], d[:, 2] = rng.uniform(-3, 3, n), rng.uniform(-0.2, 0.2, n), -1.0 if backward else 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32)


def _candidates(case, kind, backward, data):
    """-> (o, d, wanted: +1 a ray the case wants alive, -1 one it wants to fail, 0 neither), float64 geometry only."""
    rng = np.random.default_rng(sum(map(ord, case + kind)) + backward)
    z0 = data["d_sensor"] if backward else -50.0
    if case == "leaves":
        z0 = data["d_sensor"] if backward else -4.0
        o, d = _tilted(rng, 60000, z0, backward)
        lim = RADIUS * RADIUS * (1 - 1e-9)
        n_out, first_out, margin, ft = newton_outside_trips(CURV, 0.0, 0.0, lim, o, d)
        h_end = np.hypot(o[:, 0] + d[:, 0] * (-o[:, 2] / d[:, 2]), o[:, 1])
        wanted = np.where((n_out == 0) & (ft < 1e-9) & (h_end < 0.5 * RADIUS) & (np.abs(d[:, 2]) > 0.8), 1,
                          np.where((n_out >= 1) & ~first_out & (margin > 1e-3), -1, 0))
        return o, d, wanted
    lo, hi, bad_lo, bad_hi = {"tail": (0.0, 3.6, 4.2, 5.2), "nan": (0.0, 3.6, 0.0, 3.6), "stop": (0.0, 2.7, 3.2, 5.0),
                              "grazing": (0.0, 0.5 * RADIUS, 0.952 * RADIUS, 0.957 * RADIUS),
                              "tir": (0.0, 0.4 * RADIUS, 0.70 * RADIUS, 0.75 * RADIUS)}[case]
    og, dg = _parallel(rng, 1500, lo, hi, z0, backward)
    ob, db = _parallel(rng, 200, bad_lo, bad_hi, z0, backward)
    if case == "nan":
        db[:] = (F32(0.6), F32(0.8), F32(0.0))
    return np.concatenate([og, ob]), np.concatenate([dg, db]), np.concatenate([np.ones(1500, int), -np.ones(200, int)])


def _surfaces(oracle, state):
    return oracle.surfaces_from_state(state, 0.589)


def _pools(oracle, case, kind, backward):
    """The oracle sorts the candidates: (rows, data, state, good (o, d), bad (o, d))."""
    rows = _lens_rows(case, kind, backward)
    data, state = _build(rows)
    o, d, wanted = _candidates(case, kind, backward, data)
    first_good = int(np.flatnonzero(wanted == 1)[0])            # the oracle reads the direction of travel off ray 0
    order = np.concatenate([[first_good], np.delete(np.arange(len(o)), first_good)])
    o, d, wanted = o[order], d[order], wanted[order]
    rec = oracle.trace(_surfaces(oracle, state), o, d, np.ones(len(o), F32), record=True)
    alive = rec["rec_ra"] > 0                                                            # [K met, n]
    through = alive.all(axis=0)
    lost_at = np.where(through, -1, np.argmin(alive, axis=0))
    # the half of the visit that failed: the intersection leaves the position alone, Snell fails behind the commit
    before = np.concatenate([o[None], rec["rec_o"][:-1]])
    moved = np.array([(rec["rec_o"][k, i] != before[k, i]).any() if k >= 0 else False for i, k in enumerate(lost_at)])
    want_at, want_moved = {"tail": (0, False), "nan": (0, False), "stop": (0, False), "grazing": (0, True),
                           "tir": (0, True), "leaves": (0, False)}[case]
    bad = (wanted == -1) & (lost_at == want_at) & (moved == want_moved)
    good = (wanted == 1) & through
    assert good.sum() >= 128 * 9 and bad.sum() >= 9, (case, kind, backward, int(good.sum()), int(bad.sum()))
    return rows, data, state, (o[good], d[good]), (o[bad], d[bad])


def _assemble(good, bad):
    """Nine bundles of 128: all valid; one failing ray in wave 1 at each of LANES; the same in wave 0."""
    (og, dg), (ob, db) = good, bad
    o, d = og[:128 * 9].copy(), dg[:128 * 9].copy()
    dead = []
    for b, (wave, lane) in enumerate([(w, ln) for w in (1, 0) for ln in LANES], start=1):
        i = 128 * b + 64 * wave + lane
        o[i], d[i] = ob[len(dead)], db[len(dead)]
        dead.append(i)
    expect = np.ones(len(o), bool)
    expect[dead] = False
    return o, d, expect


@pytest.fixture(scope="module")
def launches(oracle):
    """(case, kind, backward) -> (data, o, d, the oracle's trace of the assembled launch): computed once, shared, left
    unchanged.  The cap is asserted here, on the CPU."""
    out = {}
    for case, kind in CASES:
        for backward in (False, True):
            rows, data, state, good, bad = _pools(oracle, case, kind, backward)
            o, d, expect = _assemble(good, bad)
            ref = oracle.trace(_surfaces(oracle, state), o, d, np.ones(len(o), F32), record=True)
            assert np.array_equal(ref["ra"] > 0, expect), (case, kind, backward, "the oracle must kill the nine rays only")
            if case == "stop":                    # ... and at the stop, so that the curved visits are entered dead
                assert not (ref["rec_ra"][0][~expect] > 0).any() and len(rows) >= 2
            waves = (ref["ra"] > 0).reshape(-1, 64).sum(axis=1)
            assert sorted(waves.tolist()) == [63] * 8 + [64] * 10
            out[case, kind, backward] = (data, o, d, ref)
    return out


def test_no_ray_leaves_the_domain_and_converges():
    rng = np.random.default_rng(5)
    found = 0
    for backward in (False, True):
        o, d = _tilted(rng, 100000, 20.0 if backward else -4.0, backward)
        n_out, first_out, margin, ft = newton_outside_trips(CURV, 0.0, 0.0, RADIUS * RADIUS * (1 - 1e-9), o, d)
        print("trips outside -> rays:", np.bincount(n_out).tolist(), "smallest |ft| of a ray that was outside:",
              float(ft[n_out > 0].min()))
        found += int(((n_out > 0) & (ft < 10e-6)).sum())
    assert found == 0


def _lens(tmp_path, data):
    from sdirt_amd import Lensgroup
    path = tmp_path / "all_valid_wave.json"
    path.write_text(json.dumps(data))
    return Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("case,kind", CASES)
def test_one_failing_lane_beside_all_valid_waves_bit_exact_against_the_oracle(launches, tmp_path, case, kind, backward,
                                                                              precision):
    from test_gpu_parity import rays_from_fixture
    data, o, d, ref = launches[case, kind, backward]
    lens = _lens(tmp_path, data)
    lens.precision = precision
    ray, _, _ = lens.trace(rays_from_fixture(o, d))
    K = len(data["surfaces"])
    assert np.array_equal(lens.trips.cache[("trace", 0.589, 0, K, not backward, precision)], ref["trips"])
    assert np.array_equal(ray.ra.cpu().numpy(), ref["ra"])
    for what, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got.view(np.int32), np.ascontiguousarray(ref[what]).view(np.int32)), (case, kind, what)


@pytest.mark.parametrize("case,kind", CASES)
def test_fused_against_two_stage_on_the_same_lenses(launches, tmp_path, case, kind):
    from sdirt_amd import _lib
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import Setup, _disc, fused, unfused
    data, o, d, ref = launches[case, kind, False]
    lens = _lens(tmp_path, data)
    # aim points: where the rays of a bundle start (they travel along the axis, or meet the vertex plane near by)
    for bundle, spp in ((0, 64), (1, 65), (4, 128), (5, 128), (8, 64)):
        s = object.__new__(Setup)
        s.lens, s.S, s.W, s.sc = lens, spp, 1, 64
        s.po = torch.tensor([[0.0, 0.0, -1500.0], [0.5, -0.25, -1200.0]], device=DEV)
        s.N = 2
        first = 128 * bundle + (64 if bundle == 8 else 0)
        aim = [np.resize(o[first:first + min(spp, 128), i], spp).astype(F32) for i in (0, 1)]
        s.x2, s.y2 = (torch.from_numpy(v)[None].contiguous().to(DEV) for v in aim)
        s.xc, s.yc = (v[None].contiguous() for v in _disc(64, 2.0 ** -7, 5))
        s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
        s.st = stream_ptr(lens.device)
        for f in (_lib.PSF_NORMALIZE, 0, _lib.PSF_STRICT_IEEE):
            a, b = fused(s, 21, f), unfused(s, 21, f)
            for what, u, v in zip(("centres", "L", "R", "primary masks", "chief-ray masks"), a, b):
                assert torch.equal(u, v), (case, kind, bundle, spp, f, what)
