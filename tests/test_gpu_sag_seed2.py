"""The sag's second quotient N c / onesf^2, onesf = 1 + sqrt(1 - a), seeded with the square of the refined 1 / onesf
(sdirt_device.hpp: sag_g_dgd, SEED2; Lean::recip, Lean::div_y, Lean::div_seeded) instead of a v_rcp_f32 of onesf^2, on
the k > -1 copies of the Newton solve, where onesf lies in [1, 2].

  the proof           sdirt_selftest_math mode 5 on the device.  Stage A: the set E of the 2^23 + 1 onesf in [1, 2] whose
                      refined reciprocal of onesf^2 differs between the two seeds.  Stage B: every member of E under all
                      2^23 numerator mantissas.  The quotients may differ for ONE pair only: onesf = 0x3fb504f3 (its
                      square rounds to the all-ones mantissa 0x3fffffff) under a power-of-two numerator.
  the guard           sdirt_lens_create marks a lens with a curved k > -1 surface whose curvature makes that numerator,
                      fl(N c), a power of two: mantissas 0x5413cc and 0x5413cd of c, at any exponent and sign.  Such a
                      handle runs the strict-IEEE kernels (sdirt_lens_strict_ieee); the curvatures two floats away, rf50mm
                      and rf35mm do not.
  adversarial rays    one-surface sphere, conic with k = 1 and asphere with four terms; curvatures 0x3ed413cd (marked),
                      its neighbours two floats away and 2^-4; semi-aperture 0.96 |R|; 64 rays PARALLEL to the axis at the
                      heights where a is 0x3f5413cd (the one preimage of that onesf) and the 8 floats on either side, and
                      where onesf is each other member of E as stage A reported it (a member that no fp32 a maps to --
                      0x3f8341ed: 1 - a is too coarse that close to a = 1 -- never occurs in a sag and has no ray; where a
                      curvature's r2 grid skips an a, the rays stand at the ones it reaches); forward and backward, Lean and strict
                      IEEE; staged sdirt_trace against the CPU oracle, bit for bit.  The oracle keeps every ray (checked on
                      the CPU before anything runs on the GPU): the ray enters the glass from air in either direction.
  fused / two-stage   sdirt_psf_lr_centered against sdirt_chief_center + sdirt_psf_lr on the forward lenses: 2 points, 64
                      and 65 samples, 64 chief rays, aim points on the lattice."""
import json

import numpy as np
import pytest
import torch

from test_gpu_surface_step import G, _ai, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ULPS = 8
BAD_ONESF = 0x3FB504F3
BAD_A = 0x3F5413CD
SEED2_WORDS, SEED2_CAP = 64, 4096


def _f(bits):
    return np.array([bits], np.uint32).view(F32)[0]


def _bits(x):
    return int(np.asarray(x, F32).reshape(1).view(np.uint32)[0])


CURVATURES = {"marked": _f(0x3ED413CD), "two_below": _f(0x3ED413CB), "two_above": _f(0x3ED413CF), "pow2": F32(2.0 ** -4)}
# kind -> (reference kind, conic, ai)
KINDS = {"sphere": ("sphere", 0.0, None), "conic_k1": ("asphere", 1.0, []), "asphere_terms": ("asphere", 0.0, _ai(43, 4))}


def _row(kind, c, backward):
    """One surface; the ray meets it coming from air in its direction of travel (into the denser glass: no total
    reflection at 0.91 R)."""
    ref_kind, k, ai = KINDS[kind]
    before, after = ("air", G[0]) if not backward else (G[0], "air")
    return (ref_kind, 0.96 / abs(float(c)), float(c), before, after, k, ai, 3.0)


def _a_of(row, x, y):
    """a as sag_g_dgd forms it: ((1 + k) * r2) * c^2 in fp32, r2 = fl(fl(x*x) + fl(y*y))."""
    c2 = F32(F32(row[2]) * F32(row[2]))
    r2 = (np.asarray(x, F32) * np.asarray(x, F32) + np.asarray(y, F32) * np.asarray(y, F32)).astype(F32)
    return ((F32(1.0 + row[5]) * r2).astype(F32) * c2).astype(F32)


def _onesf_of(a):
    a = np.asarray(a, F32)
    return (F32(1.0) + np.sqrt(F32(1.0) - a)).astype(F32)


def _preimages(onesf_bits, most=3):
    """The fp32 a in [0, 1) with fl(1 + sqrtf(1 - a)) == onesf (onesf does not increase with a): bisection and a walk."""
    target = _f(onesf_bits)
    lo, hi = 0, 0x3F800000
    while lo < hi:
        mid = (lo + hi) // 2
        if _onesf_of(_f(mid)) <= target:
            hi = mid
        else:
            lo = mid + 1
    out = []
    while lo < 0x3F800000 and _onesf_of(_f(lo)) == target and len(out) < most:
        out.append(lo)
        lo += 1
    return out


def _xy_for_r2(r2):
    """(x, y) with fl(fl(x*x) + fl(y*y)) == r2 exactly: x a little under the root, y^2 the remainder."""
    x0 = F32(np.sqrt(np.float64(r2)))
    for dx in range(0, -8, -1):
        x = (np.asarray(x0, F32).view(np.int32) + np.int32(dx)).view(F32)[()]
        xx = F32(x * x)
        if xx > r2:
            continue
        y0 = F32(np.sqrt(np.float64(r2) - np.float64(xx)))
        for dy in ((0,) if y0 == 0 else range(-2, 3)):
            y = (np.asarray(y0, F32).view(np.int32) + np.int32(dy)).view(F32)[()]
            if F32(xx + F32(y * y)) == r2:
                return x, y
    return None


def _height_for(row, a_bits):
    """(x, y) whose a is exactly the float a_bits on this surface, or None: a = fl(fl((1 + k) r2) c^2) skips floats where
    r2's grid is the coarser one (only a curvature whose square is a power of two reaches every a)."""
    scale = np.float64(F32(1.0 + row[5])) * np.float64(F32(F32(row[2]) * F32(row[2])))
    r0 = F32(np.float64(_f(a_bits)) / scale)
    for dr in (0, -1, 1, -2, 2, -3, 3):
        r2 = (np.asarray(r0, F32).view(np.int32) + np.int32(dr)).view(F32)[()]
        p = _xy_for_r2(r2)
        if p is not None and _bits(_a_of(row, p[0], p[1])) == a_bits:
            return p
    return None


def _lattice(row, members):
    """64 (x, y): a = BAD_A and the 8 floats on either side; the preimages of every other member of E; filled up with
    mirror images (squares do not see a sign, a normal does)."""
    pts, reached = [], []
    want = [BAD_A + n for n in range(-ULPS, ULPS + 1)]
    for m in members:
        if m != BAD_ONESF:
            want += _preimages(m)
    for ab in want:
        p = _height_for(row, ab)
        if p is not None:
            pts.append(p)
            reached.append(ab)
    # the exception's own a, or -- where this curvature's grid skips it -- a float next to it
    assert min(abs(ab - BAD_A) for ab in reached) <= (0 if F32(row[2]) == F32(2.0 ** -4) else 1), reached
    pts = pts[:64]
    i = 0
    while len(pts) < 64:
        x, y = pts[i]
        pts.append((-x, y) if i % 2 == 0 else (y, -x))
        i += 1
    x, y = (np.array([p[k] for p in pts], F32) for k in (0, 1))
    return x, y, reached


def _bundle(x, y, backward, d_sensor):
    o = np.stack([x, y, np.full_like(x, d_sensor if backward else -50.0)], axis=1).astype(F32)
    d = np.zeros_like(o)
    d[:, 2] = -1.0 if backward else 1.0
    return o, d


@pytest.fixture(scope="module")
def seed2():
    """sdirt_selftest_math mode 5, once: counts, the members of E, the differing pairs."""
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    out = torch.zeros(SEED2_WORDS + SEED2_CAP, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().sdirt_selftest_math(5, 0, (1 << 23) + 1, 0, dptr(out), stream_ptr(torch.device(DEV))))
    o = [int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().numpy()]
    return dict(checked=o[0], n_members=o[1], pairs=o[2], n_misses=o[3],
                misses=sorted((v >> 32, v & 0xFFFFFFFF) for v in o[4:4 + min(o[3], 16)]),
                members=sorted(o[SEED2_WORDS:SEED2_WORDS + min(o[1], SEED2_CAP)]))


def test_guard_arithmetic_on_the_cpu():
    """CPU arithmetic only: the exception's onesf has ONE preimage a, N = fma(0.5, a / sf, onesf) is one float, and
    fl(N c) is a power of two for the marked curvature and its lower neighbour alone among the six floats around it."""
    assert _preimages(BAD_ONESF, most=8) == [BAD_A]
    a = _f(BAD_A)
    sf = np.sqrt(F32(1.0) - a)
    q = F32(a / sf)
    n = F32(np.float64(0.5) * np.float64(q) + np.float64(_f(BAD_ONESF)))         # one rounding, as the fma
    assert _bits(n) == 0x401A827A
    pow2 = [cb for cb in range(0x3ED413CA, 0x3ED413D0) if _bits(F32(n * _f(cb))) & 0x7FFFFF == 0]
    assert pow2 == [0x3ED413CC, 0x3ED413CD]
    assert _bits(F32(_f(BAD_ONESF) * _f(BAD_ONESF))) == 0x3FFFFFFF


def test_seeded_second_quotient_misses_only_the_guarded_pair(seed2):
    s = seed2
    print(f"onesf checked {s['checked']:#x}; |E| = {s['n_members']}: {[hex(m) for m in s['members']]}; pairs checked "
          f"{s['pairs']:#x}; differing pairs {s['n_misses']}: {[(hex(a), hex(b)) for a, b in s['misses']]}")
    assert s["checked"] == (1 << 23) + 1
    assert s["n_members"] <= SEED2_CAP
    assert s["pairs"] == s["n_members"] << 23
    assert s["n_misses"] == len(s["misses"]) <= 1
    assert set(s["misses"]) <= {(BAD_ONESF, 0x3F800000)}          # numerator mantissa 0


def _strict(lens):
    from sdirt_amd import _lib
    return int(_lib.lib().sdirt_lens_strict_ieee(lens.dev_lens(0.589)))


def _one_surface_lens(tmp_path, row):
    from sdirt_amd import Lensgroup
    data, state = _build([row])
    path = tmp_path / "sag_seed2.json"
    path.write_text(json.dumps(data))
    return Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV), data, state


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_guard_routes_the_two_curvature_mantissas_and_nothing_else(tmp_path, kind):
    for mant in (0x5413CD, 0x5413CC):
        for exp in (0x3E800000, 0x3E800000 - (3 << 23)):           # 0.414..., and the same mantissas times 2^-3
            for sign in (0, 0x80000000):
                c = _f(sign | exp | mant)
                lens, _, _ = _one_surface_lens(tmp_path, _row(kind, c, False))
                assert _strict(lens) == 1, (kind, hex(_bits(c)))
    for cb in (0x3ED413CA, 0x3ED413CB, 0x3ED413CE, 0x3ED413CF, 0xBED413CB, 0xBED413CE, 0x3D5413CB, 0x3D5413CE):
        lens, _, _ = _one_surface_lens(tmp_path, _row(kind, _f(cb), False))
        assert _strict(lens) == 0, (kind, hex(cb))


def test_guard_leaves_a_k_le_m1_surface_and_the_shipped_lenses_alone(tmp_path):
    from conftest import load_state, make_lens
    row = ("asphere", 2.0, float(CURVATURES["marked"]), "air", G[1], -3.0, [], 3.0)    # k <= -1 keeps Lean::div
    lens, _, _ = _one_surface_lens(tmp_path, row)
    assert _strict(lens) == 0
    for name in ("rf50mm", "rf35mm"):
        assert _strict(make_lens(name, DEV, load_state(name))) == 0, name


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("curv", sorted(CURVATURES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_adversarial_heights_bit_exact_against_the_oracle(oracle, seed2, tmp_path, kind, curv, backward, precision):
    from test_gpu_parity import rays_from_fixture
    row = _row(kind, CURVATURES[curv], backward)
    x, y, reached = _lattice(row, seed2["members"])
    data, state = _build([row])
    o, d = _bundle(x, y, backward, data["d_sensor"])
    ref = oracle.trace(oracle.surfaces_from_state(state, 0.589), o, d, np.ones(len(o), F32))
    assert (ref["ra"] > 0).all(), (kind, curv, "the oracle must keep every lattice ray")      # CPU, before the GPU runs
    lens, _, _ = _one_surface_lens(tmp_path, row)
    assert _strict(lens) == (1 if curv == "marked" else 0)
    lens.precision = precision
    ray, _, _ = lens.trace(rays_from_fixture(o, d))
    assert np.array_equal(lens.trips.cache[("trace", 0.589, 0, 1, not backward, precision)], ref["trips"])
    assert np.array_equal(ray.ra.cpu().numpy(), ref["ra"])
    for what, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got.view(np.int32), np.ascontiguousarray(ref[what]).view(np.int32)), (kind, curv, what)
    assert len(np.unique(ref["d"][:, 0])) > 8           # the normal (dgd) is in what was compared
    assert len(reached) >= ULPS, reached                # a's grid is at most 2x finer than r2's: every other float at least


@pytest.mark.parametrize("curv", sorted(CURVATURES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fused_against_two_stage_on_the_adversarial_lenses(seed2, tmp_path, kind, curv):
    from sdirt_amd import _lib
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import Setup, _disc, fused, unfused
    row = _row(kind, CURVATURES[curv], False)
    lens, data, _ = _one_surface_lens(tmp_path, row)
    x, y, _ = _lattice(row, seed2["members"])
    for spp in (64, 65):
        s = object.__new__(Setup)
        s.lens, s.S, s.W, s.sc = lens, spp, 1, 64
        s.po = torch.tensor([[0.0, 0.0, -1500.0], [0.5, -0.25, -1200.0]], device=DEV)
        s.N = 2
        # aim points: the lattice itself (the 65th sample is the axis), chief rays on a disc around the axis
        aim = [np.concatenate([v, np.zeros(spp - 64, F32)]) for v in (x, y)]
        s.x2, s.y2 = (torch.from_numpy(v)[None].contiguous().to(DEV) for v in aim)
        s.xc, s.yc = (v[None].contiguous() for v in _disc(64, 2.0 ** -7, 5))
        s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
        s.st = stream_ptr(lens.device)
        for f in (_lib.PSF_NORMALIZE, 0, _lib.PSF_STRICT_IEEE):
            a, b = fused(s, 21, f), unfused(s, 21, f)
            for what, u, v in zip(("centres", "L", "R", "primary masks", "chief-ray masks"), a, b):
                assert torch.equal(u, v), (kind, curv, spp, f, what)
