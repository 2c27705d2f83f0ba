"""k_psf_lr's kernel-argument blocks (sdirt_psf.hip: SplatBlock, LoopBlock, PrimarySet) and the values its sample loops
hold in VGPRs.

Everything that moved into a block the kernel reads back with a scalar load, or into a VGPR, is a pointer, a size, a
plane or a stride: a wrong word shows as a wrong offset, not as a small error.  So every check here is bit equality
between two routes to the same numbers that decode different words, on the smallest shapes in which every moved word
matters: five points of the config-2 volume (two field corners, the axis, both ends of the depth range), a ragged last
pass (spp 1000) and three full passes (spp 1536), ks 21 -- float64 tiles: sums do not depend on their order -- and ks 65
L + R with SDIRT_PSF_DETERMINISTIC (float64 tiles in 1024-thread workgroups).

  fused / unfused     sdirt_psf_lr_centered with one workgroup per point (the CENTER instantiations: chief-ray pass inside
                      k_psf_lr) against sdirt_chief_center followed by sdirt_psf_lr on its centres (k_chief_center, then
                      the !CENTER instantiations): centres, PSFs and both convergence-mask rows
  wavelength slots    sdirt_psf_rgb_centered (W = 3: blockIdx.y offsets into x2 / y2 / xc / yc, the lens set, both trip
                      sets, masks, centres and outputs) against three single-wavelength calls
  spp cut             N = 2, spp 4096 is cut into slices (the !CENTER instantiations with nsplit > 1, k_chief_center before
                      them); uncut, the same two points are two wavelength slots' worth of one multi-wavelength launch, which
                      never cuts.  Bound below; centres bit-equal
  interleaved         SDIRT_PSF_INTERLEAVED (pstride = 2 ks^2) against separate L / R arrays
  Lean / strict IEEE  the centres of both policies (valid rays are bit-identical)
  chief-pass edges    Sc = 1, 511, 513, 1500 (fewer rays than lanes, one lane idle, a second pass with one ray, a ragged
                      third pass) through every kernel that runs the chief-ray loop or finishes a centroid

All calls run the maximal trip table (trips = NULL: SDIRT_NEWTON_MAXITER everywhere), the long Newton tables with the
periodic exit."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_state, make_lens, ulp_diff

from sdirt_amd import _lib
from sdirt_amd.basics import dptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
SC = 2048
WAVES = (0.656, 0.589, 0.486)
MS = _lib.MAX_SURFACES
EDGE = 1.0 - 1.0 / 64                     # the outermost column / row of the 32 x 32 field grid
POINTS = [[-EDGE, EDGE, -6800.0], [EDGE, -EDGE, -13400.0], [0.0, 0.0, -1000.0],
          [1.0 / 64, -1.0 / 64, -200.0], [-1.0 / 64, 1.0 / 64, -20000.0]]


@pytest.fixture(scope="module")
def lens():
    return make_lens("rf50mm", DEV, load_state("rf50mm"))


def _disc(n, radius, seed):
    """n points of a disc, float32 (x, y) on the device: pupil samples."""
    g = np.random.default_rng(seed)
    th, r = g.uniform(0, 2 * np.pi, n), radius * np.sqrt(g.uniform(0, 1, n))
    return [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV) for v in (r * np.cos(th), r * np.sin(th))]


class Setup:
    sc = SC                               # chief-ray samples per point (also of a Setup that a test fills in by hand)

    def __init__(self, lens, points, spp, seed=3, waves=1, sc=SC):
        self.lens, self.S, self.W, self.sc = lens, spp, waves, sc
        self.po = lens._points_to_object(torch.tensor(points)).clone()
        self.N = self.po.shape[0]
        pr, prc = lens.entrance_pupil()[1], lens.entrance_pupil(shrink_pupil=True)[1]
        xy = [_disc(spp, pr, seed + 10 * w) for w in range(waves)]
        cxy = [_disc(sc, prc, seed + 10 * w + 5) for w in range(waves)]
        self.x2, self.y2 = (torch.stack([p[i] for p in xy]).contiguous() for i in (0, 1))      # [W, S]
        self.xc, self.yc = (torch.stack([p[i] for p in cxy]).contiguous() for i in (0, 1))     # [W, Sc]
        self.pz, self.zs, self.ps = float(lens.entrance_pupil()[0]), float(lens.d_sensor), float(lens.pixel_size)
        self.st = stream_ptr(lens.device)


def _out(N, ks, waves=None):
    shape = (N, ks, ks) if waves is None else (N, waves, ks, ks)
    return torch.full(shape, -1.0, device=DEV), torch.full(shape, -1.0, device=DEV)


def fused(s, ks, flags=0, w=0, wvln=0.589, out=None, dp=DP):
    """sdirt_psf_lr_centered on wavelength slot w's samples -> (centres, L, R, primary masks, chief-ray masks)."""
    h = _lib.lib()
    L, R = out if out is not None else _out(s.N, ks)
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mp, mc = (torch.zeros(MS, dtype=torch.int32, device=DEV) for _ in range(2))
    dpp = _lib.DpParams(*dp)
    _lib.check(h.sdirt_psf_lr_centered(
        s.lens.dev_lens(wvln), s.lens.dev_lens(0.589), dptr(s.po), s.N, dptr(s.x2[w]), dptr(s.y2[w]), s.S, dptr(s.xc[w]),
        dptr(s.yc[w]), s.sc, s.pz, s.zs, s.ps, ks, C.byref(dpp), None, None, flags, dptr(cen), dptr(anyv), dptr(L), dptr(R),
        dptr(mp), dptr(mc), s.st))
    torch.cuda.synchronize()
    assert int(anyv.item()) == 1
    return cen, L, R, mp, mc


def unfused(s, ks, flags=0):
    """sdirt_chief_center, then sdirt_psf_lr on its centres."""
    h = _lib.lib()
    L, R = _out(s.N, ks)
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mp, mc = (torch.zeros(MS, dtype=torch.int32, device=DEV) for _ in range(2))
    dpp = _lib.DpParams(*DP)
    g = s.lens.dev_lens(0.589)
    _lib.check(h.sdirt_chief_center(g, dptr(s.po), s.N, dptr(s.xc[0]), dptr(s.yc[0]), s.sc, s.pz, s.zs, None,
                                    flags & _lib.PSF_STRICT_IEEE, dptr(cen), dptr(anyv), dptr(mc), s.st))
    _lib.check(h.sdirt_psf_lr(g, dptr(s.po), s.N, dptr(s.x2[0]), dptr(s.y2[0]), s.S, s.pz, s.zs, s.ps, ks, dptr(cen),
                              C.byref(dpp), None, flags, dptr(L), dptr(R), dptr(mp), s.st))
    torch.cuda.synchronize()
    return cen, L, R, mp, mc


def rgb(s, ks, wvlns, flags=0):
    """sdirt_psf_rgb_centered over the setup's wavelength slots -> (centres [W,N,2], L, R [N,W,ks,ks], masks [W,MS] x 2)."""
    h = _lib.lib()
    W = len(wvlns)
    L, R = _out(s.N, ks, W)
    cen = torch.full((W, s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(W, dtype=torch.int32, device=DEV)
    mp, mc = (torch.zeros((W, MS), dtype=torch.int32, device=DEV) for _ in range(2))
    dpp = _lib.DpParams(*DP)
    handles = (C.c_void_p * W)(*[s.lens.dev_lens(v) for v in wvlns])
    _lib.check(h.sdirt_psf_rgb_centered(
        handles, W, s.lens.dev_lens(0.589), dptr(s.po), s.N, dptr(s.x2), dptr(s.y2), s.S, dptr(s.xc), dptr(s.yc), s.sc, s.pz,
        s.zs, s.ps, ks, C.byref(dpp), None, None, flags, dptr(cen), dptr(anyv), dptr(L), dptr(R), dptr(mp), dptr(mc), s.st))
    torch.cuda.synchronize()
    assert bool((anyv == 1).all())
    return cen, L, R, mp, mc


def _assert_same(a, b, what):
    for name, x, y in zip(("centres", "L", "R", "primary masks", "chief-ray masks"), a, b):
        assert torch.equal(x, y), f"{what}: {name} differ, max |diff| {float((x.float() - y.float()).abs().max()):.3e}"
    assert float(a[1].sum()) > 0 and float(a[2].sum()) > 0 and bool((a[3] != 0).any()) and bool((a[4] != 0).any()), what


# one workgroup per point needs 4 x CUs points once spp passes two workgroup passes: the five points, over and over
def _points_for(spp, n_cus):
    reps = 1 if spp <= 1024 else -(-4 * n_cus // len(POINTS))
    return POINTS * reps


@pytest.fixture(scope="module")
def n_cus():
    return int(torch.cuda.get_device_properties(DEV).multi_processor_count)


@pytest.mark.parametrize("ks,spp,flags", [(21, 1000, 0), (21, 1536, 0), (65, 1000, _lib.PSF_DETERMINISTIC)])
def test_fused_against_chief_center_then_psf_lr(lens, n_cus, ks, spp, flags):
    s = Setup(lens, _points_for(spp, n_cus), spp)
    assert _lib.lib().sdirt_psf_spp_slices(s.N, spp, n_cus) == 1          # fused: the CENTER instantiations
    for f in (flags | _lib.PSF_NORMALIZE, flags):
        _assert_same(fused(s, ks, f), unfused(s, ks, f), f"ks {ks} spp {spp} flags {f}")


@pytest.mark.parametrize("ks,spp,flags", [(21, 1000, 0), (65, 1000, _lib.PSF_DETERMINISTIC)])
def test_three_wavelength_slots_against_three_calls(lens, ks, spp, flags):
    s = Setup(lens, POINTS, spp, waves=3)
    f = flags | _lib.PSF_NORMALIZE
    cen, L, R, mp, mc = rgb(s, ks, WAVES, f)
    for w, wv in enumerate(WAVES):
        one = fused(s, ks, f, w=w, wvln=wv)
        _assert_same((cen[w], L[:, w].contiguous(), R[:, w].contiguous(), mp[w], mc[w]), one, f"slot {w} ({wv} um), ks {ks}")


def test_spp_cut_against_the_uncut_launch(lens, n_cus):
    """Cut: four slices' float64 tiles are rounded to float32 and meet in global float32 atomics.  Uncut: one float64 tile,
    rounded once.  Per pixel (unnormalised, all terms >= 0, every partial sum <= the pixel <= the peak): nsplit roundings
    of the partial grids, nsplit - 1 of the additions and one of the uncut sum, each <= 2^-24 of the peak."""
    ks, spp = 21, 4096
    pts = [POINTS[0], POINTS[3]]
    nsplit = _lib.lib().sdirt_psf_spp_slices(2, spp, n_cus)
    assert nsplit > 1
    s = Setup(lens, pts, spp)
    cut = fused(s, ks, 0)
    # the same call as both slots of a two-slot launch, which keeps one workgroup per (point, slot)
    s2 = Setup(lens, pts, spp, waves=2)
    s2.x2[1], s2.y2[1], s2.xc[1], s2.yc[1] = s2.x2[0], s2.y2[0], s2.xc[0], s2.yc[0]
    cen, L, R, mp, mc = rgb(s2, ks, (0.589, 0.589), 0)
    assert torch.equal(L[:, 0], L[:, 1]) and torch.equal(R[:, 0], R[:, 1]) and torch.equal(cen[0], cen[1])
    assert torch.equal(cut[0], cen[0]), "centres of the cut call"
    assert torch.equal(cut[3], mp[0]) and torch.equal(cut[4], mc[0]), "convergence masks of the cut call"
    for side, (a, b) in (("L", (cut[1], L[:, 0])), ("R", (cut[2], R[:, 0]))):
        peak = b.amax(dim=(1, 2), keepdim=True)
        bound = 2 * nsplit * 2.0 ** -24
        d = float(((a - b).abs() / peak).max())
        print(f"{side}: nsplit {nsplit}, max |cut - uncut| / peak {d:.3e} (bound {bound:.3e})")
        assert float(peak.min()) > 0 and d <= bound, (side, d, bound)


def test_interleaved_against_separate_outputs(lens):
    ks, spp = 21, 1000
    s = Setup(lens, POINTS, spp)
    f = _lib.PSF_NORMALIZE
    sep = fused(s, ks, f)
    both = torch.full((s.N, 2, ks, ks), -1.0, device=DEV)
    il = fused(s, ks, f | _lib.PSF_INTERLEAVED, out=(both[:, 0], both[:, 1]))
    _assert_same((il[0], both[:, 0].contiguous(), both[:, 1].contiguous(), il[3], il[4]), sep, "interleaved")


def test_lean_and_strict_ieee_centres(lens):
    s = Setup(lens, POINTS, 1000)
    lean, ieee = fused(s, 21, _lib.PSF_NORMALIZE), fused(s, 21, _lib.PSF_NORMALIZE | _lib.PSF_STRICT_IEEE)
    assert torch.equal(lean[0], ieee[0]), float((lean[0] - ieee[0]).abs().max())
    lean_u, ieee_u = unfused(s, 21, 0), unfused(s, 21, _lib.PSF_STRICT_IEEE)
    assert torch.equal(lean_u[0], ieee_u[0]) and torch.equal(lean_u[0], lean[0])


# ------------------------------------------------------------------ the edges of the chief-ray loop
def _centre_entry(s, flags, slope):
    """sdirt_chief_center / sdirt_chief_center_slope -> (centres, any_valid, chief-ray masks)."""
    h = _lib.lib()
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mc = torch.zeros(MS, dtype=torch.int32, device=DEV)
    head = (s.lens.dev_lens(0.589), dptr(s.po), s.N, dptr(s.xc[0]), dptr(s.yc[0]), s.sc, s.pz, s.zs, None, flags, dptr(cen))
    if slope:
        sl = torch.full((s.N, 2), float("nan"), dtype=torch.float64, device=DEV)
        _lib.check(h.sdirt_chief_center_slope(*head, dptr(sl), dptr(anyv), dptr(mc), s.st))
    else:
        _lib.check(h.sdirt_chief_center(*head, dptr(anyv), dptr(mc), s.st))
    torch.cuda.synchronize()
    return cen, anyv, mc


def _staged(s, flags):
    """The same chief rays by the staged chain: sdirt_sample_rays, sdirt_trace2sensor on the green lens,
    sdirt_center_from_rays -> ((centres, any_valid, the trace's masks), the sensor-plane bundle)."""
    from sdirt_amd.basics import Ray
    h = _lib.lib()
    ray = Ray.empty((s.sc, s.N), 0.589, DEV)
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mc = torch.zeros(MS, dtype=torch.int32, device=DEV)
    _lib.check(h.sdirt_sample_rays(dptr(s.po), s.N, dptr(s.xc[0]), dptr(s.yc[0]), s.sc, s.pz, ray.c_rays(), s.st))
    _lib.check(h.sdirt_trace2sensor(s.lens.dev_lens(0.589), None, flags, s.zs, ray.c_rays(), ray.c_rays(), ray.numel,
                                    dptr(mc), s.st))
    _lib.check(h.sdirt_center_from_rays(ray.c_rays(), s.sc, s.N, dptr(cen), dptr(anyv), s.st))
    torch.cuda.synchronize()
    return (cen, anyv, mc), ray


@pytest.mark.parametrize("sc", [1, 511, 513, 1500])
def test_chief_ray_pass_at_the_edges_of_its_loop(lens, sc):
    """Everything else here runs the chief-ray pass at Sc = 2048, a whole number of passes of a 512- and of a 1024-thread
    workgroup.  The routes of 512 threads under the strict-IEEE policy -- sdirt_chief_center, sdirt_chief_center_slope,
    sdirt_psf_lr_centered with r <= 0.5 and with r > 0.5 (the indexed sample loop) -- trace the same rays, add them in the
    same tree and finish alike: centres, any_valid and the chief-ray masks are the same bits.  So are the centres and
    any_valid of the Lean fused call (the pinned sample loop; valid rays are bit-identical under both policies).
    Another tree -- 1024 threads (ks 65, SDIRT_PSF_DETERMINISTIC), 256 threads (sdirt_center_from_rays over the staged
    trace of the same rays) -- gives float64 sums that differ in their last bits: against the float64 sums of the staged
    rays taken here, either cast to float32 may fall one step either way and the quotient rounds once more, 4 steps of
    the centre; masks and any_valid are equal."""
    ieee = _lib.PSF_STRICT_IEEE
    s = Setup(lens, POINTS, 1000, sc=sc)
    ref = _centre_entry(s, ieee, slope=False)
    assert int(ref[1].item()) == 1 and bool((ref[2] != 0).any()) and bool(torch.isfinite(ref[0]).all())

    def three(f):                                             # (centres, any_valid, chief-ray masks) of a fused call
        return f[0], torch.ones(1, dtype=torch.int32, device=DEV), f[4]    # (fused() has asserted any_valid == 1)
    same_tree = {
        "sdirt_chief_center_slope": _centre_entry(s, ieee, slope=True),
        "fused, r 0.5": three(fused(s, 21, ieee)),
        "fused, r 0.65": three(fused(s, 21, ieee, dp=(*DP[:3], 0.65))),
    }
    for name, got in same_tree.items():
        for what, x, y in zip(("centres", "any_valid", "chief-ray masks"), got, ref):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"Sc {sc}, {name}: {what} differ"
    lean = fused(s, 21, 0)
    assert torch.equal(lean[0].view(torch.int32), ref[0].view(torch.int32)), f"Sc {sc}, Lean fused: centres differ"

    staged, ray = _staged(s, ieee)
    ra = ray.ra.double()                                                         # [Sc, N]
    sx, sy = ((ray.o[..., i] * ray.ra).double().sum(0) for i in (0, 1))          # the kernels' fp32 products, float64 sums
    den = ra.sum(0).float() + torch.tensor(1e-9, dtype=torch.float32, device=DEV)
    want = torch.stack([-(sx.float() / den), -(sy.float() / den)], 1)
    assert bool(torch.isfinite(want).all()) and float(ra.sum(0).min()) >= 1.0
    other_tree = {
        "1024 threads": three(fused(s, 65, ieee | _lib.PSF_DETERMINISTIC)),
        "sdirt_center_from_rays": staged,
    }
    for name, got in {"512 threads": ref, **other_tree}.items():
        d = int(ulp_diff(got[0].cpu().numpy(), want.cpu().numpy()).max())
        print(f"Sc {sc}, {name}: centres {d} float32 steps from the float64 sums")
        assert d <= 4, (sc, name, d)
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), f"Sc {sc}, {name}: any_valid or masks differ"
