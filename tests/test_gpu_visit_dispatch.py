"""The dispatch of a surface visit (sdirt_device.hpp: visit_bits, surface_reaction, curved_hit, refract; sdirt_trace.hpp:
trace_ray) on prescriptions in which every class of visit follows every other.

A visit takes one of four paths through its first half and one of four through its second, by bits the host wrote into
the surface's flags word; the next surface's constants and its entry of the trip table are fetched between the halves.
What can go wrong is wave-uniform and whole: a visit that runs the previous surface's path, reads its trip count or a
constant of it, or picks the wrong copy of the Newton loop.  Nothing of that is a small error, so everything here is
bit equality, on the smallest bundles that have a full wave and a wave with one live lane.

  classes             stop plane, refracting plane, sphere, conic k > -1, conic k <= -1, asphere with terms: an Euler
                      circuit of the complete directed graph on the six, so each of the 30 ordered pairs occurs as two
                      neighbouring surfaces (stop -> asphere, asphere -> sphere, conic k <= -1 -> refracting plane and
                      refracting plane -> conic k > -1 among them).  Curvature signs, glasses, conic constants and the
                      polynomial's coefficients change from surface to surface.
  lenses              that circuit (31 surfaces), a lens of one surface (a sphere; nothing to prefetch) and one of
                      SDIRT_MAX_SURFACES surfaces (every byte of the trip words in use).
  trip tables         the reference's own and the maximal one through Lensgroup.trace (trip_policy 'reference', 'max');
                      hand-written ones through sdirt_trace with 0, 1, 4, 5 and 10 trips on neighbouring surfaces -- no
                      loop, the plain loop up to its longest, the loop with the periodic exit from its shortest -- against
                      the CPU oracle forced to the same counts; the negative (per-wave adaptive) form of the same tables
                      in the fused comparison, where both sides are kernels.
  staged trace        k_trace, forward and backward, Lean and strict IEEE, against the CPU oracle: positions,
                      directions, weights, obliquity (bit patterns of the live rays), trip tables; the convergence
                      masks of a hand-written table hold no bit of a trip that did not run.
  fused / two-stage   sdirt_psf_lr_centered against sdirt_chief_center + sdirt_psf_lr: centres, both mask rows and the
                      ks 21 PSFs (float64 tiles: the sums do not depend on their order), 2 points, 64 and 65 samples,
                      64 chief rays.

No case may pass on dead rays: each asserts that the oracle alone keeps at least 90 % of its rays alive to the last
surface."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GLASSES = ["1.51680/64.2", "1.80518/25.4", "1.67270/32.1", "1.53110/55.9"]
CLASSES = ("stop", "window", "sphere", "conic_gt", "conic_le", "asphere")
AI_SCALES = (2e-4, 2e-5, 2e-7, 1e-9, 1e-11, 1e-13)
DP = (0.78, 1.44, 0.3, 0.5)
SC = 64


def euler_circuit(n):
    """Vertices of an Euler circuit of the complete directed graph on n vertices (Hierholzer): n (n - 1) + 1 of them,
    every ordered pair of different vertices once as neighbours."""
    out = {v: [w for w in range(n) if w != v][::-1] for v in range(n)}
    stack, path = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def rows_for(classes):
    """One row of test_gpu_surface_step._build per class index; the medium alternates between air and a glass that
    changes every time, a stop stands in whatever medium it finds."""
    rows, medium, glass = [], "air", 0
    for i, ci in enumerate(classes):
        cls = CLASSES[ci]
        sign = 1.0 if i % 2 == 0 else -1.0
        c = sign * (0.004 + 0.0015 * (i % 7))
        if cls == "stop":
            rows.append(("plane", 7.0 + 0.25 * (i % 3), 0.0, medium, medium, 0.0, None, 0.6))
            continue
        if medium == "air":
            after, glass = GLASSES[glass % len(GLASSES)], glass + 1
        else:
            after = "air"
        if cls == "window":
            rows.append(("plane", 8.0 + 0.5 * (i % 3), 0.0, medium, after, 0.0, None, 0.7))
        elif cls == "sphere":
            rows.append(("sphere", 8.0 + 0.5 * (i % 3), c, medium, after, 0.0, None, 0.8))
        elif cls == "conic_gt":
            rows.append(("asphere", 8.5, c, medium, after, (-0.6, 0.0, 0.45)[i % 3], [], 0.9))
        elif cls == "conic_le":
            rows.append(("asphere", 8.5, c, medium, after, (-1.0, -1.8)[i % 2], [], 0.7))
        else:
            rng = np.random.default_rng(100 + i)
            deg = (6, 3, 1, 4)[i % 4]
            rows.append(("asphere", 8.5, c, medium, after, (0.0, 0.3, -1.4)[i % 3],
                         [float(rng.normal(0, s)) for s in AI_SCALES[:deg]], 0.8))
        medium = after
    return rows


def _lenses():
    from sdirt_amd import _lib
    circuit = euler_circuit(len(CLASSES))
    assert len(circuit) == 31 and len({(a, b) for a, b in zip(circuit, circuit[1:])}) == 30
    pairs = {(CLASSES[a], CLASSES[b]) for a, b in zip(circuit, circuit[1:])}
    assert {("stop", "asphere"), ("asphere", "sphere"), ("conic_le", "window"), ("window", "conic_gt")} <= pairs
    longest = (circuit + circuit[1:] + circuit[1:])[:_lib.MAX_SURFACES]
    assert len(longest) == _lib.MAX_SURFACES == 64
    return {"circuit": circuit, "one_surface": [CLASSES.index("sphere")], "max_surfaces": longest}


def hand_tables(classes):
    """Two trip tables for a class sequence: 0, 1, 4, 5, 10 in turn on the spheres and 4, 5, 10 in turn on the other
    curved surfaces (a sphere's validity is its own test, so it keeps its rays with any count; Newton's own validity on
    the others needs the residual below 10e-6, which no trip or one trip do not reach), 0 on planes, which run no
    loop.  The second table is shifted by two: every curved surface meets two counts, and neighbours sit in different
    copies of the loop."""
    out = []
    for shift in (0, 2):
        t, j = [], shift
        for ci in classes:
            if CLASSES[ci] in ("stop", "window"):
                t.append(0)
                continue
            t.append((0, 1, 4, 5, 10)[j % 5] if CLASSES[ci] == "sphere" else (4, 5, 10)[j % 3])
            j += 1
        out.append(np.asarray(t, np.int32))
    return out


def _bundle(rng, n, backward, z_last):
    """A narrow, nearly collimated bundle: every ray passes every aperture of these weak lenses."""
    o = np.zeros((n, 3), np.float32)
    o[:, :2] = rng.uniform(-2.0, 2.0, (n, 2))
    o[:, 2] = z_last + 20.0 if backward else -40.0
    d = np.zeros((n, 3), np.float64)
    d[:, :2] = rng.normal(0, 0.01, (n, 2))
    d[:, 2] = -1.0 if backward else 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


N_RAYS = 2 * 65            # two full waves and two rays of a third


@pytest.fixture(scope="module")
def cases(oracle):
    """lens name -> dict(data, classes, K, tables, runs[(backward, table index or policy)] = (o, d, oracle's trace)):
    computed once, shared, left unchanged."""
    from test_gpu_surface_step import _build
    out = {}
    for i, (name, classes) in enumerate(_lenses().items()):
        data, state = _build(rows_for(classes))
        surf = oracle.surfaces_from_state(state, 0.589)
        K = len(classes)
        curved = np.array([CLASSES[c] not in ("stop", "window") for c in classes])
        tables = {"reference": None, "max": np.where(curved, 10, 0).astype(np.int32)}
        tables.update({f"hand{j}": t for j, t in enumerate(hand_tables(classes))})
        rng = np.random.default_rng(700 + i)
        runs = {}
        for backward in (False, True):
            o, d = _bundle(rng, N_RAYS, backward, data["surfaces"][-1]["z"])
            for tname, t in tables.items():
                ref = oracle.trace(surf, o, d, np.ones(len(o), np.float32), trips=t)
                assert ref["ra"].mean() >= 0.9, (name, backward, tname, "the oracle keeps too few rays alive")
                runs[(backward, tname)] = (o, d, ref)
        out[name] = dict(data=data, classes=classes, K=K, tables=tables, runs=runs, state=state)
    return out


def _lens(tmp_path, data, precision):
    from sdirt_amd import Lensgroup
    path = tmp_path / "visit_dispatch.json"
    path.write_text(json.dumps(data))
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    lens.precision = precision
    return lens


def _assert_rays(ray, ref, what):
    assert np.array_equal(ray.ra.cpu().numpy(), ref["ra"]), what
    live = ref["ra"] > 0
    for field, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got, ref[field]), (field, what)
        # bit patterns: the sign of a zero counts
        assert np.array_equal(got[live].view(np.int32), np.ascontiguousarray(ref[field][live]).view(np.int32)), (field, what)


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("policy", ["reference", "max"])
@pytest.mark.parametrize("name", ["circuit", "one_surface", "max_surfaces"])
def test_trace_against_the_oracle_under_both_trip_policies(cases, tmp_path, name, policy, backward, precision):
    from test_gpu_parity import rays_from_fixture
    case = cases[name]
    o, d, ref = case["runs"][(backward, policy)]
    lens = _lens(tmp_path, case["data"], precision)
    lens.trip_policy = policy
    ray, _, _ = lens.trace(rays_from_fixture(o, d))
    if policy == "reference":
        key = ("trace", 0.589, 0, case["K"], not backward, precision)
        assert np.array_equal(lens.trips.cache[key], ref["trips"]), (name, backward, precision)
    _assert_rays(ray, ref, (name, policy, backward, precision))


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("name", ["circuit", "one_surface", "max_surfaces"])
def test_trace_with_hand_written_trip_tables_against_the_oracle(cases, tmp_path, name, backward, precision):
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    from test_gpu_parity import rays_from_fixture
    case = cases[name]
    K = case["K"]
    lens = _lens(tmp_path, case["data"], precision)
    masks = {}
    for table in ("hand0", "hand1"):
        trips = case["tables"][table]
        o, d, ref = case["runs"][(backward, table)]
        assert np.array_equal(ref["trips"], trips)                     # the oracle ran the forced counts
        ray = rays_from_fixture(o, d)
        mask = torch.zeros(_lib.MAX_SURFACES, dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib().sdirt_trace(lens.dev_lens(0.589), 0, K, 1 if backward else 0,
                                          (C.c_int32 * K)(*trips.tolist()), lens._math_flags(), ray.c_rays(), ray.numel,
                                          dptr(mask), stream_ptr(lens.device)))
        torch.cuda.synchronize()
        ray._mark_traced()
        _assert_rays(ray, ref, (name, table, backward, precision))
        # bit j + 1 of a surface's mask: trip j had an open ray somewhere.  Only bits the table ran can be set, and a
        # surface without trips has none
        m = masks[table] = mask.cpu().numpy().astype(np.int64)
        for k in range(K):
            assert m[k] & ~((2 << int(trips[k])) - 2) == 0, (name, table, k, hex(m[k]), int(trips[k]))
    # A trip's open flag does not depend on how many trips follow it, and the rays reach a surface in the same state
    # under both tables only on the FIRST curved surface of the pass: there the masks agree on the trips both ran (a
    # stale trip count, or a mask taken from the neighbour's copy of the loop, shows here)
    t0, t1 = case["tables"]["hand0"], case["tables"]["hand1"]
    order = range(K - 1, -1, -1) if backward else range(K)
    k = next(k for k in order if case["tables"]["max"][k] != 0)
    both = (2 << int(min(t0[k], t1[k]))) - 2
    assert masks["hand0"][k] & both == masks["hand1"][k] & both, (name, backward, precision, k)


# ---- fused against the two-stage launches ---------------------------------------------------------------------------
class _Setup:
    pass


def _setup(lens, data, spp, seed):
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import _disc
    s = _Setup()
    s.lens, s.S = lens, spp
    s.po = torch.tensor([[0.0, 0.0, -1500.0], [12.0, -9.0, -1200.0]], device=DEV)
    s.N = 2
    s.x2, s.y2 = _disc(spp, 1.6, seed)
    s.xc, s.yc = _disc(SC, 0.4, seed + 5)
    s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
    s.st = stream_ptr(lens.device)
    return s


def _tab(t):
    return None if t is None else (C.c_int32 * len(t))(*[int(v) for v in t])


def _fused(s, ks, flags, tp, tc):
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr
    from test_gpu_psf_kernarg_blocks import MS, _out
    L, R = _out(s.N, ks)
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mp, mc = (torch.zeros(MS, dtype=torch.int32, device=DEV) for _ in range(2))
    dpp = _lib.DpParams(*DP)
    g = s.lens.dev_lens(0.589)
    _lib.check(_lib.lib().sdirt_psf_lr_centered(
        g, g, dptr(s.po), s.N, dptr(s.x2), dptr(s.y2), s.S, dptr(s.xc), dptr(s.yc), SC, s.pz, s.zs, s.ps, ks,
        C.byref(dpp), _tab(tp), _tab(tc), flags, dptr(cen), dptr(anyv), dptr(L), dptr(R), dptr(mp), dptr(mc), s.st))
    torch.cuda.synchronize()
    assert int(anyv.item()) == 1
    return cen, L, R, mp, mc


def _unfused(s, ks, flags, tp, tc):
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr
    from test_gpu_psf_kernarg_blocks import MS, _out
    L, R = _out(s.N, ks)
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mp, mc = (torch.zeros(MS, dtype=torch.int32, device=DEV) for _ in range(2))
    dpp = _lib.DpParams(*DP)
    g = s.lens.dev_lens(0.589)
    _lib.check(_lib.lib().sdirt_chief_center(g, dptr(s.po), s.N, dptr(s.xc), dptr(s.yc), SC, s.pz, s.zs, _tab(tc),
                                             flags & _lib.PSF_STRICT_IEEE, dptr(cen), dptr(anyv), dptr(mc), s.st))
    _lib.check(_lib.lib().sdirt_psf_lr(g, dptr(s.po), s.N, dptr(s.x2), dptr(s.y2), s.S, s.pz, s.zs, s.ps, ks, dptr(cen),
                                       C.byref(dpp), _tab(tp), flags, dptr(L), dptr(R), dptr(mp), s.st))
    torch.cuda.synchronize()
    return cen, L, R, mp, mc


def _oracle_alive(oracle, case, s):
    """Share of the setup's rays, primary and chief, that the oracle alone keeps alive through the lens."""
    surf = oracle.surfaces_from_state(case["state"], 0.589)
    po = s.po.cpu().numpy()
    share = []
    for x, y in ((s.x2, s.y2), (s.xc, s.yc)):
        o, d, ra, _ = oracle.sample_rays(po, x.cpu().numpy(), y.cpu().numpy(), s.pz)
        share.append(float(oracle.trace(surf, o.reshape(-1, 3), d.reshape(-1, 3), ra.reshape(-1))["ra"].mean()))
    return min(share)


@pytest.mark.parametrize("spp", [64, 65])
@pytest.mark.parametrize("name", ["circuit", "one_surface", "max_surfaces"])
def test_fused_against_two_stage_on_every_table(cases, oracle, tmp_path, name, spp):
    from sdirt_amd import _lib
    from test_gpu_psf_kernarg_blocks import _assert_same
    case = cases[name]
    lens = _lens(tmp_path, case["data"], "lean")
    s = _setup(lens, case["data"], spp, seed=3 + spp)
    assert _oracle_alive(oracle, case, s) >= 0.9
    n_cus = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    assert _lib.lib().sdirt_psf_spp_slices(s.N, spp, n_cus) == 1          # fused: the CENTER instantiations
    h0, h1 = case["tables"]["hand0"], case["tables"]["hand1"]
    tables = [(None, None), (h0, h1), (h1, h0), (-h0, -h1), (-h1, -h0), (case["tables"]["max"], -case["tables"]["max"])]
    curved = case["tables"]["max"] != 0
    for tp, tc in tables:
        for flags in (0, _lib.PSF_STRICT_IEEE):
            a, b = _fused(s, 21, flags, tp, tc), _unfused(s, 21, flags, tp, tc)
            what = f"{name}, spp {spp}, flags {flags}, primary table {None if tp is None else tp.tolist()}"
            if tp is not None and not ((np.abs(tp)[curved] > 0).any() and (np.abs(tc)[curved] > 0).any()):
                # a lens whose only curved surface runs no trip in one of the passes has no mask bit to show there
                for x, y in zip(a, b):
                    assert torch.equal(x, y), what
                continue
            _assert_same(a, b, what)
