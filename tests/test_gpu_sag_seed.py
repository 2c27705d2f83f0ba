"""The conic sag's quotient a / sqrt(1 - a) seeded with the root's own v_rsq_f32 (sdirt_device.hpp: sag_g_dgd, Lean,
INSIDE; Lean::sqrt_pos_rsq, Lean::div_seeded) instead of a v_rcp_f32 of the root.

The quotient's last bit DOES depend on the seed for a handful of a; what reads it,
G(a) = fma(0.5, a / sf, 1 + sf) with sf = sqrt_pos(1 - a), must not.  sf is a function of a alone, so the claim is about
one fp32 and is settled by trying all of them, on the device (v_rsq_f32 and v_rcp_f32 are the hardware's):

  every fp32 a        sdirt_selftest_math mode 4 over all 2^32 bit patterns: no a whose G differs where 1 - a is a
                      positive normal float, none elsewhere that is not NaN under both seeds; the number of a whose bare
                      quotient differs is printed.
  absorbed pairs      a = 2^-23 and a = 2^-24 are where sf = 1 - 2^-24 has an all-ones mantissa under a power-of-two
                      numerator, the one combination at which the seeded quotient can miss the correctly rounded one, and
                      where 1 + sf = 2.0f swallows the miss.  One-surface lenses with c = 2^-4 (c^2 = 2^-8 exactly),
                      rays PARALLEL to the axis landing at (2^-8, 2^-8) (r^2 = 2^-15, a = 2^-23 on a sphere) and at
                      (2^-8, 0) (r^2 = 2^-16, a = 2^-24), and at the 8 floats on either side of each height: sphere, conic
                      with k > -1, conic with k <= -1, asphere with polynomial terms; forward and backward, Lean and strict
                      IEEE; staged sdirt_trace against the CPU oracle, bit for bit, 64 rays per case.  The oracle keeps
                      every lattice ray alive (checked on the CPU before anything runs on the GPU).
  fused / two-stage   sdirt_psf_lr_centered against sdirt_chief_center + sdirt_psf_lr on those lenses: 2 points, 64 and
                      65 samples, 64 chief rays, aim points on and around the two heights.

Nothing here states new behaviour: all of it also holds for a library that seeds the division with v_rcp_f32."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from test_gpu_surface_step import G, _ai, _build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ULPS = 8
CURV = 2.0 ** -4
H = F32(2.0 ** -8)

# (kind, semi-aperture, curvature, glass before, glass after, conic, ai, distance to the next vertex).  1 + k is a power
# of two everywhere, so a = ((1 + k) * r2) * c^2 is a power of two at the two heights: 2^-23 and 2^-24 with k = 0,
# 2^-22 and 2^-23 with k = 1, -2^-22 and -2^-23 with k = -3 (a <= 0: the radicand is >= 1, nothing to absorb)
LENSES = {
    "sphere": ("sphere", 1.0, CURV, "air", G[0], 0.0, None, 3.0),
    "conic_k_gt_m1": ("asphere", 1.0, CURV, "air", G[0], 1.0, [], 3.0),
    "conic_k_le_m1": ("asphere", 1.0, CURV, "air", G[1], -3.0, [], 3.0),
    "asphere_terms": ("asphere", 1.0, CURV, "air", G[0], 0.0, _ai(41, 4), 3.0),
}


def _step(x, n):
    """The float n floats above (n < 0: below) the positive fp32 x."""
    return (np.asarray(x, F32).view(np.int32) + np.asarray(n, np.int32)).view(F32)


def _heights():
    """64 (x, y): the two heights, the 8 floats on either side of each coordinate that is not zero (x alone, and x and y
    together), and the mirror images of the first 13 (squares do not see a sign, a normal does)."""
    n = np.arange(-ULPS, ULPS + 1)
    x = np.concatenate([_step(H, n), _step(H, n), _step(H, n)])
    y = np.concatenate([np.full(len(n), H), _step(H, n), np.zeros(len(n), F32)])
    x, y = np.concatenate([x, -x[ULPS - 6:ULPS + 7]]), np.concatenate([y, -y[ULPS - 6:ULPS + 7]])
    assert len(x) == 64
    return x.astype(F32), y.astype(F32)


def _bundle(backward, d_sensor):
    x, y = _heights()
    o = np.stack([x, y, np.full_like(x, d_sensor if backward else -50.0)], axis=1).astype(F32)
    d = np.zeros_like(o)
    d[:, 2] = -1.0 if backward else 1.0
    return o, d


def _a_of(row, x, y):
    """a as sag_g_dgd forms it: ((1 + k) * r2) * c^2 in fp32, r2 = fl(fl(x*x) + fl(y*y))."""
    c2 = F32(F32(row[2]) * F32(row[2]))
    r2 = (x * x + y * y).astype(F32)
    return ((F32(1.0 + row[5]) * r2).astype(F32) * c2).astype(F32)


def test_lattice_holds_the_absorbed_pairs():
    """CPU arithmetic only: the lattice reaches a = 2^-23 and a = 2^-24, the root there is 1 - 2^-24 and 1 + root is
    2.0f, whose half-ulp (2^-23) exceeds half the quotient's whole value -- G is 2.0f for the quotient and both of its
    neighbours."""
    x, y = _heights()
    for name in ("sphere", "asphere_terms"):
        a = _a_of(LENSES[name], x, y)
        assert F32(2.0 ** -23) in a and F32(2.0 ** -24) in a, name
    assert F32(2.0 ** -23) in _a_of(LENSES["conic_k_gt_m1"], x, y)
    assert F32(-2.0 ** -23) in _a_of(LENSES["conic_k_le_m1"], x, y)
    for a in (F32(2.0 ** -23), F32(2.0 ** -24)):
        sf = np.sqrt(F32(1.0) - a)                                       # correctly rounded, as sqrt_pos is
        assert sf.view(np.uint32) == 0x3F7FFFFF and F32(F32(1.0) + sf) == F32(2.0)
        q = F32(a / sf)
        for qq in (_step(q, -1), q, _step(q, 1)):
            assert F32(np.float64(0.5) * np.float64(qq) + 2.0) == F32(2.0)      # one rounding, as the fma


def test_seeded_quotient_is_invisible_on_every_fp32():
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    out = torch.zeros(9, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().sdirt_selftest_math(4, 0, 1 << 32, 0, dptr(out), stream_ptr(torch.device(DEV))))
    o = [int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().numpy()]
    print(f"checked {o[0]:#x}; G differs, radicand positive normal: {o[1]} (first a {o[4]:#x}); G differs elsewhere, "
          f"not NaN under both: {o[2]} (first a {o[5]:#x}); bare quotient differs: {o[3]} (first a {o[6]:#x})")
    assert o[0] == 1 << 32
    assert o[1] == 0 and o[2] == 0
    assert o[4] == o[5] == 0xFFFFFFFFFFFFFFFF and o[7] == o[8] == 0


@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("name", sorted(LENSES))
def test_absorbed_pair_lattice_bit_exact_against_the_oracle(oracle, tmp_path, name, backward, precision):
    from sdirt_amd import Lensgroup
    from test_gpu_parity import rays_from_fixture
    data, state = _build([LENSES[name]])
    o, d = _bundle(backward, data["d_sensor"])
    ref = oracle.trace(oracle.surfaces_from_state(state, 0.589), o, d, np.ones(len(o), F32))
    assert (ref["ra"] > 0).all(), (name, "the oracle must keep every lattice ray")       # CPU, before the GPU runs
    path = tmp_path / "sag_seed.json"
    path.write_text(json.dumps(data))
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    lens.precision = precision
    ray, _, _ = lens.trace(rays_from_fixture(o, d))
    assert np.array_equal(lens.trips.cache[("trace", 0.589, 0, 1, not backward, precision)], ref["trips"])
    assert np.array_equal(ray.ra.cpu().numpy(), ref["ra"])
    for what, got in (("o", ray.o), ("d", ray.d), ("obliq", ray.obliq)):
        got = np.ascontiguousarray(got.cpu().numpy())
        assert np.array_equal(got.view(np.int32), np.ascontiguousarray(ref[what]).view(np.int32)), (name, what)
    # the refracted directions are not all the same: the normal (dgd) is in what was compared
    assert len(np.unique(ref["d"][:, 0])) > 8


@pytest.mark.parametrize("name", sorted(LENSES))
def test_fused_against_two_stage_on_the_lattice_lenses(tmp_path, name):
    from sdirt_amd import Lensgroup, _lib
    from sdirt_amd.basics import stream_ptr
    from test_gpu_psf_kernarg_blocks import Setup, _disc, fused, unfused
    data, _ = _build([LENSES[name]])
    path = tmp_path / "sag_seed_psf.json"
    path.write_text(json.dumps(data))
    lens = Lensgroup(str(path), sensor_res=(512, 768), post_computation=False, device=DEV)
    x, y = _heights()
    for spp in (64, 65):
        s = object.__new__(Setup)
        s.lens, s.S, s.W, s.sc = lens, spp, 1, 64
        s.po = torch.tensor([[0.0, 0.0, -1500.0], [0.5, -0.25, -1200.0]], device=DEV)
        s.N = 2
        # aim points: the lattice itself (the 65th sample is the axis), chief rays on a disc around it
        aim = [np.concatenate([v, np.zeros(spp - 64, F32)]) for v in (x, y)]
        s.x2, s.y2 = (torch.from_numpy(v)[None].contiguous().to(DEV) for v in aim)
        s.xc, s.yc = (v[None].contiguous() for v in _disc(64, 2.0 ** -7, 5))
        s.pz, s.zs, s.ps = 0.0, float(data["d_sensor"]), 0.25
        s.st = stream_ptr(lens.device)
        for f in (_lib.PSF_NORMALIZE, 0, _lib.PSF_STRICT_IEEE):
            a, b = fused(s, 21, f), unfused(s, 21, f)
            for what, u, v in zip(("centres", "L", "R", "primary masks", "chief-ray masks"), a, b):
                assert torch.equal(u, v), (name, spp, f, what)
            assert float(a[1].sum()) > 0 and float(a[2].sum()) > 0, (name, spp, f)
