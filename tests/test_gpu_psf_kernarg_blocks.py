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

All calls run the maximal trip table (trips = NULL: SDIRT_NEWTON_MAXITER everywhere), the long Newton tables with the
periodic exit."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_state, make_lens

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
    def __init__(self, lens, points, spp, seed=3, waves=1):
        self.lens, self.S, self.W = lens, spp, waves
        self.po = lens._points_to_object(torch.tensor(points)).clone()
        self.N = self.po.shape[0]
        pr, prc = lens.entrance_pupil()[1], lens.entrance_pupil(shrink_pupil=True)[1]
        xy = [_disc(spp, pr, seed + 10 * w) for w in range(waves)]
        cxy = [_disc(SC, prc, seed + 10 * w + 5) for w in range(waves)]
        self.x2, self.y2 = (torch.stack([p[i] for p in xy]).contiguous() for i in (0, 1))      # [W, S]
        self.xc, self.yc = (torch.stack([p[i] for p in cxy]).contiguous() for i in (0, 1))     # [W, Sc]
        self.pz, self.zs, self.ps = float(lens.entrance_pupil()[0]), float(lens.d_sensor), float(lens.pixel_size)
        self.st = stream_ptr(lens.device)


def _out(N, ks, waves=None):
    shape = (N, ks, ks) if waves is None else (N, waves, ks, ks)
    return torch.full(shape, -1.0, device=DEV), torch.full(shape, -1.0, device=DEV)


def fused(s, ks, flags=0, w=0, wvln=0.589, out=None):
    """sdirt_psf_lr_centered on wavelength slot w's samples -> (centres, L, R, primary masks, chief-ray masks)."""
    h = _lib.lib()
    L, R = out if out is not None else _out(s.N, ks)
    cen = torch.full((s.N, 2), -1.0, device=DEV)
    anyv = torch.zeros(1, dtype=torch.int32, device=DEV)
    mp, mc = (torch.zeros(MS, dtype=torch.int32, device=DEV) for _ in range(2))
    dpp = _lib.DpParams(*DP)
    _lib.check(h.sdirt_psf_lr_centered(
        s.lens.dev_lens(wvln), s.lens.dev_lens(0.589), dptr(s.po), s.N, dptr(s.x2[w]), dptr(s.y2[w]), s.S, dptr(s.xc[w]),
        dptr(s.yc[w]), SC, s.pz, s.zs, s.ps, ks, C.byref(dpp), None, None, flags, dptr(cen), dptr(anyv), dptr(L), dptr(R),
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
    _lib.check(h.sdirt_chief_center(g, dptr(s.po), s.N, dptr(s.xc[0]), dptr(s.yc[0]), SC, s.pz, s.zs, None,
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
        handles, W, s.lens.dev_lens(0.589), dptr(s.po), s.N, dptr(s.x2), dptr(s.y2), s.S, dptr(s.xc), dptr(s.yc), SC, s.pz,
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
