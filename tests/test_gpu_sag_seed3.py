"""The conic sag's quotient a / sqrt(1 - a), seeded with the root's own v_rsq_f32, WITHOUT the two fma that refine the
seed (sdirt_device.hpp: Lean::div_seeded_once; sag_g_dgd under SEED2, the k > -1 copies of the Newton solve): q0 = a r,
q = fma(fma(-sf, q0, a), r, q0).

That is no division in general; what reads it, G(a) = fma(0.5, q, 1 + sf), must not see the difference.  sf and r are
functions of a alone, so the claim is about one fp32 and the device tries all of them:

  every fp32 a        sdirt_selftest_math mode 6 over all 2^32 bit patterns.  The gate as it came out on MI355X, which is
                      the variant that was built: NO a >= 0 whose G differs where 1 - a is a positive normal float, none
                      outside that domain that is not NaN under both forms -- and ONE a < 0 that does differ,
                      0xc525406d, which is why k <= -1 (a <= 0), the normals and the recording trace keep
                      Lean::div_seeded.  The bare quotient differs at the ten a of QUOT; the hardware's v_rsq_f32 at
                      PROBE, the one argument a CPU restatement with a seed one float low told apart, is the correctly
                      rounded one.
  CPU restatement     the two forms in numpy fp32 (fma through float64) under the correctly rounded seed and its two
                      neighbours: at the nine a >= 0 of QUOT G takes the same bits for q and for BOTH neighbours of q
                      (absorbed whatever the seed does); at 0xc525406d and at PROBE it does not, and a seed one float
                      low shows there.
  adversarial rays    one-surface lenses with c = 2^-4 (c^2 = 2^-8: a = (1 + k) r2 2^-8 is exact, every a is reached):
                      sphere, conic k = 1, conic k = -3 (a < 0: the same heights, the side that keeps div_seeded) and an
                      asphere with four terms; rays PARALLEL to the axis landing where |a| is PROBE, each a >= 0 of QUOT,
                      and the 8 floats on either side of each: 170 heights, three bundles of 64 rays; forward and
                      backward, Lean and strict IEEE; staged sdirt_trace against the CPU oracle, bit for bit.  The oracle
                      keeps every ray (checked on the CPU before anything runs on the GPU).
  fused / two-stage   sdirt_psf_lr_centered against sdirt_chief_center + sdirt_psf_lr on the forward lenses: 2 points, 64
                      and 65 samples, 64 chief rays, aim points on each bundle.

Only the mode-6 case states new behaviour; the rest also holds for a library that refines the seed."""
import json

import numpy as np
import pytest
import torch

from test_gpu_surface_step import G, _ai, _build
from test_gpu_sag_seed2 import _a_of, _bits, _bundle, _f, _height_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ULPS = 8
CURV = 2.0 ** -4
PROBE = 0x3DC39C73
# the a whose bare quotient differs between the forms, as mode 6 lists them on MI355X (profiles/sag_seed3)
QUOT = [0x343FFFFF, 0x34DFFFFD, 0x35B5554D, 0x3647AE01, 0x37C1513E, 0x382148EA, 0x38A45ED6, 0x38E0CE80, 0x3C46AF22,
        0xC525406D]
QUOT_POS = [a for a in QUOT if a < 0x80000000]
G_BREAKS = 0xC525406D
# kind -> (reference kind, glass, conic, ai)
KINDS = {"sphere": ("sphere", G[0], 0.0, None), "conic_k1": ("asphere", G[0], 1.0, []),
         "conic_km3": ("asphere", G[1], -3.0, []), "asphere_terms": ("asphere", G[0], 0.0, _ai(43, 4))}
N_BUNDLES = 3


def _row(kind, backward):
    """One surface, semi-aperture 0.96 |R|; the ray meets it coming from air in its direction of travel."""
    ref_kind, glass, k, ai = KINDS[kind]
    before, after = ("air", glass) if not backward else (glass, "air")
    return (ref_kind, 0.96 / CURV, CURV, before, after, k, ai, 3.0)


def _lattice(row):
    """N_BUNDLES x 64 (x, y): |a| = PROBE, each a >= 0 of QUOT, and the 8 floats on either side of each -- c^2 and
    |1 + k| are powers of two, so every one of them is reached; the last bundle is filled up with mirror images (squares
    do not see a sign, a normal does)."""
    sign = 0x80000000 if row[5] < -1.0 else 0
    pts = []
    for centre in [PROBE] + QUOT_POS:
        for n in range(-ULPS, ULPS + 1):
            want = sign | (centre + n)
            # _height_for scales by (1 + k) c^2 in float64: a negative a gives a negative r2, so aim at |a| with |1 + k|
            p = _height_for(row[:5] + (abs(1.0 + row[5]) - 1.0,) + row[6:], centre + n)
            assert p is not None, hex(want)
            assert _bits(_a_of(row, p[0], p[1])) == want, hex(want)
            pts.append(p)
    assert len(pts) == 17 * (1 + len(QUOT_POS)) <= 64 * N_BUNDLES
    i = 0
    while len(pts) < 64 * N_BUNDLES:
        x, y = pts[i]
        pts.append((-x, y) if i % 2 == 0 else (y, -x))
        i += 1
    x, y = (np.array([p[k] for p in pts], F32).reshape(N_BUNDLES, 64) for k in (0, 1))
    return x, y


def _step(x, n):
    return (np.asarray(x, F32).reshape(1).view(np.int32) + np.int32(n)).view(F32)[0]


def _fma(a, b, c):
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _forms(a, seed_offset):
    """(q refined twice, q not refined, 1 + sf) in fp32 as the device forms them, the seed `seed_offset` floats from the
    correctly rounded 1 / sqrt(1 - a)."""
    x = F32(F32(1.0) - a)
    r = _step(F32(1.0 / np.sqrt(np.float64(x))), seed_offset)
    s = F32(x * r)
    sf = _fma(_fma(-s, s, x), F32(F32(0.5) * r), s)                              # Lean::sqrt_pos_rsq
    assert _bits(sf) == _bits(np.sqrt(x))
    y = _fma(_fma(-sf, r, F32(1.0)), r, r)
    q0 = F32(a * y)
    q_two = _fma(_fma(-sf, q0, a), y, q0)                                        # Lean::div_seeded
    p0 = F32(a * r)
    q_once = _fma(_fma(-sf, p0, a), r, p0)                                       # Lean::div_seeded_once
    return q_two, q_once, F32(F32(1.0) + sf)


def test_forms_and_absorption_on_the_cpu():
    for ab in QUOT_POS:
        for off in (-1, 0, 1):
            q_two, q_once, onesf = _forms(_f(ab), off)
            assert abs(_bits(q_two) - _bits(q_once)) <= 1, (hex(ab), off)
            g = {_bits(_fma(F32(0.5), _step(q_two, n), onesf)) for n in (-1, 0, 1)}
            assert len(g) == 1 and _bits(_fma(F32(0.5), q_once, onesf)) in g, (hex(ab), off)
    for ab in (G_BREAKS, PROBE):
        q_two, q_once, onesf = _forms(_f(ab), 0)
        assert _bits(q_two) == _bits(q_once), hex(ab)                           # nothing to absorb under the exact seed
        q_two, q_once, onesf = _forms(_f(ab), -1)
        assert _bits(q_two) != _bits(q_once), hex(ab)
        assert _bits(_fma(F32(0.5), q_two, onesf)) != _bits(_fma(F32(0.5), q_once, onesf)), hex(ab)
    x, y = _lattice(_row("sphere", False))
    a = _a_of(_row("sphere", False), x.ravel(), y.ravel()).view(np.uint32)
    assert {PROBE, *QUOT_POS} <= set(int(v) for v in a)
    a = _a_of(_row("conic_km3", False), x.ravel(), y.ravel())
    assert (a <= 0).all()


def test_unrefined_seed_is_invisible_on_every_fp32_a_ge_0():
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    out = torch.zeros(_lib.SELFTEST_LIST_WORDS + _lib.SELFTEST_LIST_CAP, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().sdirt_selftest_math(6, 0, 1 << 32, 0, dptr(out), stream_ptr(torch.device(DEV))))
    s = _lib.decode_seed_once(out.cpu().numpy())
    print({k: ([hex(v) for v in s[k]] if k == "quot" else s[k]) for k in s})
    assert s["checked"] == 1 << 32
    # the gate, for the variant that was built: the form runs where a >= 0 (or a is outside the domain) and nowhere else
    assert s["g_pos"] == 0 and s["g_outside"] == 0
    assert s["first_g"][0] is None and s["first_g"][2] is None
    # ... and may not run on a < 0: were this 0, sag_g_dgd could use the form for every caller
    assert s["g_neg"] == 1 and s["first_g"][1] == G_BREAKS
    assert s["n_quot"] == len(QUOT) and s["quot"] == sorted(QUOT)
    exact = F32(1.0 / np.sqrt(np.float64(F32(F32(1.0) - _f(PROBE)))))
    assert s["seed_bits"] - _bits(exact) == s["seed_offset"] == 0


def _one_surface_lens(tmp_path, row):
    from sdirt_amd import Lensgroup
    data, state = _build([row])
    path = tmp_path / "sag_seed3.json"
    path.write_text(json.dumps(data))
    return Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV), data, state


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("bundle", range(N_BUNDLES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_adversarial_heights_bit_exact_against_the_oracle(oracle, tmp_path, kind, bundle, backward, precision):
    from test_gpu_parity import rays_from_fixture
    row = _row(kind, backward)
    x, y = _lattice(row)
    data, state = _build([row])
    o, d = _bundle(x[bundle], y[bundle], backward, data["d_sensor"])
    ref = oracle.trace(oracle.surfaces_from_state(state, 0.589), o, d, np.ones(len(o), F32))
    assert (ref["ra"] > 0).all(), (kind, bundle, "the oracle must keep every lattice ray")    # CPU, before the GPU runs
    lens, _, _ = _one_surface_lens(tmp_path, row)
    lens.precision = precision
    ray, _, _ = lens.trace(rays_from_fixture(o, d))
    assert np.array_equal(lens.trips.cache[("trace", 0.589, 0, 1, not backward, precision)], ref["trips"])
    assert np.array_equal(ray.ra.cpu().numpy(), ref["ra"])
    for what, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got.view(np.int32), np.ascontiguousarray(ref[what]).view(np.int32)), (kind, bundle, what)
    assert len(np.unique(ref["d"][:, 0])) > 8           # the normal (dgd) is in what was compared


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fused_against_two_stage_on_the_adversarial_lenses(tmp_path, kind):
    from sdirt_amd import _lib
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import Setup, _disc, fused, unfused
    row = _row(kind, False)
    lens, data, _ = _one_surface_lens(tmp_path, row)
    xs, ys = _lattice(row)
    for bundle, spp in ((0, 64), (1, 65), (2, 64)):
        s = object.__new__(Setup)
        s.lens, s.S, s.W, s.sc = lens, spp, 1, 64
        s.po = torch.tensor([[0.0, 0.0, -1500.0], [0.5, -0.25, -1200.0]], device=DEV)
        s.N = 2
        # aim points: the bundle itself (the 65th sample is the axis), chief rays on a disc around the axis
        aim = [np.concatenate([v[bundle], np.zeros(spp - 64, F32)]) for v in (xs, ys)]
        s.x2, s.y2 = (torch.from_numpy(v)[None].contiguous().to(DEV) for v in aim)
        s.xc, s.yc = (v[None].contiguous() for v in _disc(64, 2.0 ** -7, 5))
        s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
        s.st = stream_ptr(lens.device)
        for f in (_lib.PSF_NORMALIZE, 0, _lib.PSF_STRICT_IEEE):
            a, b = fused(s, 21, f), unfused(s, 21, f)
            for what, u, v in zip(("centres", "L", "R", "primary masks", "chief-ray masks"), a, b):
                assert torch.equal(u, v), (kind, bundle, spp, f, what)
