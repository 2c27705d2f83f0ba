"""The edges of one surface visit (sdirt_device.hpp: surface_reaction, curved_hit, newton_k, refract): the aperture
test of a stop, the domain test of an asphere, and lanes of one wave that die at different surfaces.  Everything is bit
equality against the CPU oracle (staged trace) or between the fused kernel and the two-stage launches; nothing here
states new behaviour.

  aperture lattice     a stop plane first, two spheres behind it, rays PARALLEL to the axis: the intersection with the
                       plane is x + t * 0, the ray's own (x, y), exactly.  (x, y) are chosen on the CPU so that the fp32
                       x*x + y*y takes EVERY float within 8 ulps on either side of X, the largest fp32 whose correctly
                       rounded root is <= the stop's radius -- the test sqrt(x^2 + y^2) <= r (surfaces.py:421) flips
                       between X and the float above it, which is where an aperture test without the root can go wrong.
                       X is not fl(r * r): the test asserts how far above it lies.
  domain-edge lattice  the same lattice around lim_tight of an asphere that is the FIRST surface: k > -1 with and without
                       polynomial terms and a domain (lim_loose) that ends inside the aperture, k <= -1 with and without
                       terms (lim_tight is the aperture).  Next to lim_loose the conic's radicand 1 - a goes to zero.
  lanes that die       4096 rays whose heights are swept so that the oracle loses rays at four or more different
                       surfaces; and the fused kernel against sdirt_chief_center + sdirt_psf_lr on that prescription.

Forward, the lattice is what the stop (the asphere) sees.  Backward the same rays start behind the lens and reach the
stop last, refracted: no lattice then, but still rays on either side of the edge, compared bit for bit.
Every staged case traces at most 4096 rays; the fused case 5 points x (700 + 2048) rays."""
import json

import numpy as np
import pytest
import torch

from test_gpu_surface_step import G, _ai, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ULPS = 8


def _step(x, n):
    """The float n floats above (n < 0: below) the positive fp32 x."""
    return (np.asarray(x, F32).view(np.int32) + np.int32(n)).view(F32)


def _largest_square_under(r):
    """The largest fp32 X with sqrt(X) <= r, correctly rounded root (numpy's fp32 sqrt is): stepped from fl(r * r)."""
    r = F32(r)
    x = F32(r * r)
    while np.sqrt(x) > r:
        x = _step(x, -1)
    while np.sqrt(_step(x, 1)) <= r:
        x = _step(x, 1)
    return F32(x)


def _lattice(centre, per_target, seed):
    """(x, y), fp32, such that fl(fl(x*x) + fl(y*y)) takes each of the 2 * ULPS + 1 floats around `centre` at least
    `per_target` times -> (x [n], y [n], the sums [n]).  Found by search: y anywhere in [0, 0.6 sqrt(centre)], x the
    rounded root of what is left, tried with its neighbours."""
    rng = np.random.default_rng(seed)
    centre = F32(centre)
    xs, ys = [], []
    for off in range(-ULPS, ULPS + 1):
        target = _step(centre, off)
        found = 0
        while found < per_target:
            y = rng.uniform(0.0, 0.6 * np.sqrt(float(centre)), 4096).astype(F32)
            x0 = np.sqrt(np.maximum(np.float64(target) - np.float64(y) ** 2, 0.0)).astype(F32)
            for dx in (0, -1, 1, -2, 2):
                x = _step(x0, dx)
                hit = (x * x + y * y) == target                     # fp32 products, fp32 sum
                take = np.flatnonzero(hit)[:per_target - found]
                xs.append(x[take]); ys.append(y[take])
                found += len(take)
                if found >= per_target:
                    break
    x, y = np.concatenate(xs), np.concatenate(ys)
    sign = rng.integers(0, 2, (2, len(x))) * 2 - 1                  # all four quadrants: squares do not see the sign
    x, y = (x * sign[0]).astype(F32), (y * sign[1]).astype(F32)
    return x, y, x * x + y * y


def _assert_covers(sums, centre):
    got = set(np.asarray(sums, F32).view(np.int32).tolist())
    want = set(_step(F32(centre), np.arange(-ULPS, ULPS + 1)).view(np.int32).tolist())
    assert want <= got, f"the lattice misses {len(want - got)} of the {len(want)} floats around {float(centre)!r}"


def _parallel_bundle(x, y, radius, backward, d_sensor, seed, fill=512):
    """The lattice rays plus `fill` rays spread over [0, 1.3 radius], all parallel to the axis."""
    rng = np.random.default_rng(seed)
    rad, th = radius * 1.3 * np.sqrt(rng.uniform(0, 1, fill)), rng.uniform(0, 2 * np.pi, fill)
    x = np.concatenate([x, (rad * np.cos(th)).astype(F32)])
    y = np.concatenate([y, (rad * np.sin(th)).astype(F32)])
    o = np.stack([x, y, np.full_like(x, d_sensor if backward else -50.0)], axis=1).astype(F32)
    d = np.zeros_like(o)
    d[:, 2] = -1.0 if backward else 1.0
    return o, d


def _trace_and_compare(oracle, tmp_path, data, state, o, d, backward, precision, what):
    """k_trace against the oracle: trip table, weights, and the bit patterns of positions, directions, obliquity."""
    from sdirt_amd import Lensgroup
    from test_gpu_parity import rays_from_fixture
    ref = oracle.trace(oracle.surfaces_from_state(state, 0.589), o, d, np.ones(len(o), F32))
    live = ref["ra"] > 0
    print(f"{what}: {int(live.sum())} live, {int((~live).sum())} dead of {len(live)}")
    assert live.any() and (~live).any(), (what, "needs live and dead rays")
    path = tmp_path / "visit_edges.json"
    path.write_text(json.dumps(data))
    K = len(data["surfaces"])
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    lens.precision = precision
    ray, _, _ = lens.trace(rays_from_fixture(o, d))
    key = ("trace", 0.589, 0, K, not backward, precision)
    assert np.array_equal(lens.trips.cache[key], ref["trips"]), (what, "trip table")
    got_ra = ray.ra.cpu().numpy()
    print(f"{what}: weights differ on {int((got_ra != ref['ra']).sum())} rays")
    assert np.array_equal(got_ra, ref["ra"]), (what, "weights")
    for name, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got, ref[name]), (what, name)
        assert np.array_equal(got[live].view(np.int32), np.ascontiguousarray(ref[name][live]).view(np.int32)), \
            (what, name, "bit patterns of the live rays")
    return ref


# ---- 1. the stop's aperture ------------------------------------------------------------------------------------------
RADII = [5.0, 4.3, 7.123, 2.0, 0.37]


def _stop_first(radius):
    return _build([("plane", radius, 0.0, "air", "air", 0.0, None, 2.0),
                   ("sphere", 9.5, 0.030, "air", G[0], 0.0, None, 3.0),
                   ("sphere", 9.5, -0.025, G[0], "air", 0.0, None, 2.0)])


@pytest.fixture(scope="module")
def stop_lattices():
    """radius -> (X, x, y): computed once, shared, left unchanged."""
    out = {}
    for i, radius in enumerate(RADII):
        X = _largest_square_under(radius)
        x, y, sums = _lattice(X, 24, 100 + i)
        _assert_covers(sums, X)
        out[radius] = (X, x, y)
    return out


def test_the_largest_square_under_a_radius_is_not_the_rounded_square():
    above = {r: int(_largest_square_under(r).view(np.int32)) - int(F32(F32(r) * F32(r)).view(np.int32)) for r in RADII}
    print(above)
    assert all(v >= 0 for v in above.values()) and above[0.37] == 0 and all(above[r] >= 1 for r in (5.0, 4.3, 7.123, 2.0))


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("radius", RADII)
def test_aperture_lattice_bit_exact_against_the_oracle(oracle, stop_lattices, tmp_path, radius, backward, precision):
    X, x, y = stop_lattices[radius]
    data, state = _stop_first(radius)
    assert np.float32(state["surfaces"][0]["r"]) == F32(radius)
    o, d = _parallel_bundle(x, y, radius, backward, data["d_sensor"], 7)
    ref = _trace_and_compare(oracle, tmp_path, data, state, o, d, backward, precision,
                             f"stop r = {radius}, {'backward' if backward else 'forward'}, {precision}")
    if not backward:
        # the lattice rays live or die by the stop alone (the spheres behind it are wide): x^2 + y^2 <= X
        n = len(x)
        assert np.array_equal(ref["ra"][:n] > 0, (x * x + y * y) <= X)


# ---- 2. the asphere's domain -----------------------------------------------------------------------------------------
def _lim_tight(c, k, semi):
    """make_dev_surface's fp32 arithmetic (surfaces.py:728,739)."""
    c, k = F32(c), F32(k)
    r2_lim = F32(float(semi) * float(semi))
    if not k > -1:
        return r2_lim
    rc = F32(F32(1.0) / F32(c * c)) * F32(1.0 - 1e-9)
    return min(r2_lim, F32(rc / F32(F32(1.0) + k)))


EDGES = {
    # c = 0.12, k = 0.5: the conic ends at r^2 = 46.3 (r = 6.8), inside the semi-aperture of 9
    "k_gt_m1_terms": ("asphere", 9.0, 0.12, "air", G[0], 0.5, _ai(11, 4), 6.0),
    "k_gt_m1_conic": ("asphere", 9.0, 0.12, "air", G[0], 0.5, [], 6.0),
    "k_le_m1_terms": ("asphere", 6.0, 0.05, "air", G[1], -1.4, _ai(12, 6), 4.0),
    "k_le_m1_conic": ("asphere", 6.0, 0.05, "air", G[1], -1.0, [], 4.0),
}


@pytest.fixture(scope="module")
def edge_lattices():
    out = {}
    for i, (name, row) in enumerate(sorted(EDGES.items())):
        lim = _lim_tight(row[2], row[5], row[1])
        if row[5] > -1:
            assert lim < F32(row[1] * row[1]), "the domain must end inside the aperture"
        x, y, sums = _lattice(lim, 24, 200 + i)
        _assert_covers(sums, lim)
        out[name] = (lim, x, y)
    return out


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_domain_edge_lattice_bit_exact_against_the_oracle(oracle, edge_lattices, tmp_path, name, backward, precision):
    lim, x, y = edge_lattices[name]
    row = EDGES[name]
    data, state = _build([row, ("sphere", 9.5, -0.02, row[4], "air", 0.0, None, 2.0)])
    o, d = _parallel_bundle(x, y, float(np.sqrt(lim)), backward, data["d_sensor"], 9)
    _trace_and_compare(oracle, tmp_path, data, state, o, d, backward, precision,
                       f"{name}, {'backward' if backward else 'forward'}, {precision}")


# ---- 3. lanes that die at different surfaces -------------------------------------------------------------------------
NARROWING = [
    ("sphere", 9.0, 0.030, "air", G[1], 0.0, None, 3.0),
    ("sphere", 7.5, -0.025, G[1], "air", 0.0, None, 2.0),
    ("plane", 5.0, 0.0, "air", "air", 0.0, None, 2.0),
    ("asphere", 3.9, 0.030, "air", G[0], -0.6, _ai(21, 6), 2.5),
    ("asphere", 3.3, -0.020, G[0], "air", -1.8, [], 1.5),
    ("sphere", 2.9, 0.020, "air", G[3], 0.0, None, 2.5),
    ("asphere", 2.4, -0.030, G[3], "air", 0.0, _ai(22, 3), 2.0),
]


def _swept_bundle(n, seed):
    """Heights swept from the axis to beyond the first aperture, lane by lane (neighbours in a wave differ), with a
    small random tilt."""
    rng = np.random.default_rng(seed)
    h = np.linspace(0.0, 10.0, n)
    th = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([h * np.cos(th), h * np.sin(th), np.full(n, -50.0)], axis=1).astype(F32)
    d = np.zeros((n, 3))
    d[:, :2] = rng.normal(0, 0.05, (n, 2))
    d[:, 2] = 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    perm = rng.permutation(n)                                       # every wave holds rays of every fate
    return o[perm], d.astype(F32)[perm]


@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_lanes_that_die_at_different_surfaces_trace_bit_exact(oracle, tmp_path, precision):
    data, state = _build(NARROWING)
    o, d = _swept_bundle(4096, 31)
    surf = oracle.surfaces_from_state(state, 0.589)
    rec = oracle.trace(surf, o, d, np.ones(len(o), F32), record=True)["rec_ra"]          # [K, n]
    lost_at = np.where((rec > 0).all(axis=0), -1, np.argmin(rec > 0, axis=0))
    ks = sorted(set(lost_at.tolist()) - {-1})
    print("rays lost at surface:", {k: int((lost_at == k).sum()) for k in ks}, "through:", int((lost_at == -1).sum()))
    assert len(ks) >= 4, ks
    first_wave = set(lost_at[:64].tolist())
    assert len(first_wave - {-1}) >= 3 and -1 in first_wave, "one wave must hold several fates"
    _trace_and_compare(oracle, tmp_path, data, state, o, d, False, precision, f"narrowing, {precision}")


def test_lanes_that_die_fused_against_two_stage(tmp_path):
    from sdirt_amd import Lensgroup, _lib
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import SC, Setup, _assert_same, _disc, fused, unfused
    spp = 700
    data, _ = _build(NARROWING)
    path = tmp_path / "visit_edges_psf.json"
    path.write_text(json.dumps(data))
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    s = object.__new__(Setup)
    s.lens, s.S, s.W = lens, spp, 1
    s.po = torch.tensor([[0.0, 0.0, -1500.0], [40.0, -30.0, -1200.0], [-25.0, 35.0, -2500.0], [5.0, 5.0, -600.0],
                         [0.0, 60.0, -3000.0]], device=DEV)
    s.N = s.po.shape[0]
    # aim discs wider than the stop: rays of one wave die at the first two spheres, the stop and behind it
    s.x2, s.y2 = (v[None].contiguous() for v in _disc(spp, 8.0, 3))
    s.xc, s.yc = (v[None].contiguous() for v in _disc(SC, 6.0, 8))
    s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
    s.st = stream_ptr(lens.device)
    n_cus = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    assert _lib.lib().sdirt_psf_spp_slices(s.N, spp, n_cus) == 1          # fused: the CENTER instantiations
    for f in (_lib.PSF_NORMALIZE, 0, _lib.PSF_STRICT_IEEE):
        _assert_same(fused(s, 21, f), unfused(s, 21, f), f"narrowing, flags {f}")
