"""Photometric dual-pixel PSFs on the GPU: the energy of every point (sdirt_dp_energy, sdirt_dp_energy_grad;
DESIGN.md 7j) against the float64 restatement (tests/energy_f64.py, which tests/test_energy_cpu.py ties to
tests/splat_f64.py), through monte_carlo.dp_energy, Lensgroup.psf_lr(energy=True), the recorded trace and
Lensgroup.psf_volume(photometric=True).

The fuzz runs on the synthetic sensor-plane rays of tests/test_gpu_dp_grad.py (every launch shape of FUZZ_TABLE, r on
both sides of 0.5, both precisions).  make_case kills the rays a float64 reference cannot judge inside the splat's window
only, the energy counts every live ray: the rays splat_f64.fragile_x flags among ALL live rays get ra = 0 here, before the
kernel or the restatement sees them, under the same cap.

Bars: per point and component |kernel - float64| <= 1e-5 x sum|terms| (the bar the splat's fuzz holds for the same
fp32 weights), forward and backward; per ray 1e-5 of the larger of |term| and the row's largest term."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import load_state, make_lens
from energy_f64 import energy_f64, energy_grad_f64, energy_scale_f64, x_tan_f64
from splat_f64 import fragile_x
from test_gpu_dp_grad import FRAGILE_CAP, FUZZ_TABLE, fuzz_case, make_case
from test_gpu_trace_grad import _abi

from sdirt_amd import _lib
from sdirt_amd.basics import DEFAULT_WAVE, dptr, stream_ptr
from sdirt_amd.monte_carlo import _flags, dp_energy, forward_integral_lr
from sdirt_amd.render_psf import local_dp_psf_render_volume, photometric_scale, volume_segment_tables
from sdirt_amd.trace_grad import N_COLUMNS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
BAR = 1e-5
FEW_RAYS = 400
SPP = 960                   # below the spp at which a small batch is cut along spp: the grids repeat bit for bit


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _ncu():
    return int(torch.cuda.get_device_properties(DEV).multi_processor_count)


def _slices(N, S):
    return int(_lib.lib().sdirt_forward_integral_grad_slices(N, S, _ncu()))


def _ray(case):
    from test_gpu_parity import rays_from_fixture
    ray = rays_from_fixture(case["o"], case["d"])
    ray.ra = _t(case["ra"])
    return ray


def _kill_fragile(case):
    """ra = 0 for every live ray fragile_x flags, in the window or not; asserts the cap."""
    ox, oy, dx, dz, ra = case["rays"]
    live = ra != 0
    extra = fragile_x(x_tan_f64(dx, dz, ra), case["h"], case["f"], case["w"], case["r"]) & live
    n_live, n_extra = int(live.sum()), int(extra.sum())
    assert n_extra <= (2 if n_live < FEW_RAYS else FRAGILE_CAP * n_live), (n_extra, n_live)
    ra = ra * (~extra)
    case["rays"][4], case["ra"] = ra, ra.numpy()
    case["n_live_all"], case["n_fragile_all"] = n_live, n_extra
    return case


@functools.lru_cache(maxsize=None)
def _fuzz(seed):
    """One fuzz case with its float64 answers, computed once and shared by the forward and the backward fuzz."""
    case = _kill_fragile(fuzz_case(seed))
    _, _, dx, dz, ra = case["rays"]
    dp = tuple(case[k] for k in "hfwr")
    case["E"], case["E_scale"] = energy_f64(dx, dz, ra, *dp), energy_scale_f64(dx, dz, ra, *dp)
    case["G"] = torch.randn((case["N"], 3), dtype=torch.float64, generator=torch.Generator().manual_seed(100 + seed))
    case["grad"] = energy_grad_f64(dx, dz, ra, *dp, case["G"])
    return case


def _dpp(case):
    return _lib.DpParams(*[float(case[k]) for k in "hfwr"])


def _abi_energy(case, ray, n_slices=None, dp="case", fill=float("nan")):
    """sdirt_dp_energy called directly -> (status, partial [N, rows, 3] float64 on the device)."""
    S, N = case["S"], case["N"]
    ns = max(_slices(N, S), 1)
    rows = ns if n_slices is None else max(ns, n_slices) + 1
    partial = torch.full((max(N, 1), rows, 3), fill, dtype=torch.float64, device=DEV)
    dpp = _dpp(case) if dp == "case" else dp
    rc = _lib.lib().sdirt_dp_energy(ray.c_rays(), S, N, C.byref(dpp) if dpp is not None else None, _flags(case["precision"]),
                                    dptr(partial), ns if n_slices is None else n_slices, stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, partial


def _abi_energy_grad(case, ray, G, partial=True, ray_grad=None, accumulate=0, n_slices=None, dp="case", fill=float("nan")):
    """sdirt_dp_energy_grad called directly -> (status, partial [N, slices, 3] float64 on the device or None)."""
    S, N = case["S"], case["N"]
    ns = max(_slices(N, S), 1)
    rows = ns if n_slices is None else max(ns, n_slices) + 1
    part = torch.full((max(N, 1), rows, 3), fill, dtype=torch.float64, device=DEV) if partial else None
    dpp = _dpp(case) if dp == "case" else dp
    ge = G.to(DEV, torch.float64).contiguous()
    rc = _lib.lib().sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dpp) if dpp is not None else None,
                                         _flags(case["precision"]), dptr(ge), dptr(part), ns if n_slices is None else n_slices,
                                         dptr(ray_grad), accumulate, stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, part


def _worst(got, want, scale):
    """max |got - want| / scale; where the scale is 0 (no ray contributes) the kernel's value must be exactly 0."""
    got, want, scale = (torch.as_tensor(a).double().reshape(-1) for a in (got, want, scale))
    assert bool(torch.isfinite(got).all())
    dead = scale == 0
    assert bool((got[dead] == 0).all()), "a value where no ray contributes"
    return float(((got - want).abs()[~dead] / scale[~dead]).max()) if bool((~dead).any()) else 0.0


def _sn(row, case):
    """A row of a [., n_rays] buffer (point-major) as [S, N]."""
    return row.reshape(case["N"], case["S"]).t()


# ------------------------------------------------------------------ the forward fuzz
@pytest.mark.parametrize("seed", range(len(FUZZ_TABLE)))
def test_energy_kernel_against_the_float64_restatement(seed):
    case = _fuzz(seed)
    ray = _ray(case)
    dp = tuple(case[k] for k in "hfwr")
    got = dp_energy(ray, dp, case["precision"])
    assert got.shape == (case["N"], 3) and got.dtype == torch.float64 and got.grad_fn is None
    worst = _worst(got[:, :2].cpu(), case["E"][:, :2], case["E_scale"][:, :2])
    print(f"energy fuzz {seed}: S {case['S']} N {case['N']} r {case['r']:.4f} {case['precision']} live {case['n_live_all']} "
          f"fragile among all live rays {case['n_fragile_all']} ({case['n_fragile_all'] / max(case['n_live_all'], 1):.1e}): "
          f"worst |kernel - float64| / sum|terms| = {worst:.2e}")
    assert worst <= BAR
    assert torch.equal(got[:, 2].cpu(), case["rays"][4].double().sum(0))          # 0 / 1 weights: an exact count
    # the C entry: the same bits as the Python call, twice
    rc, p1 = _abi_energy(case, ray)
    rc2, p2 = _abi_energy(case, ray)
    assert rc == 0 == rc2 and torch.equal(p1, p2) and torch.equal(p1.sum(1), got)
    assert p1.shape[1] == _slices(case["N"], case["S"])


def test_fractional_weights_and_a_point_without_a_live_ray():
    """ra in [0.25, 1): column 2 is sum(ra) within n 2^-53 relative (float64 additions of fp32 numbers in another order
    than the restatement's); a point all of whose rays are dead gives exactly 0 in every column."""
    for k, (r, prec) in enumerate([(0.45, "lean"), (0.62, "ieee")]):
        case = make_case(np.random.default_rng(30 + k), 1500, 4, 21, 0.00431, 0.7, 1.5, 0.35, r, prec, weights=True)
        case["ra"][:, 2] = 0.0
        case["rays"][4] = torch.from_numpy(case["ra"])
        case = _kill_fragile(case)
        assert len(np.unique(case["ra"])) > 100
        _, _, dx, dz, ra = case["rays"]
        dp = tuple(case[k_] for k_ in "hfwr")
        got = dp_energy(_ray(case), dp, prec).cpu()
        want, scale = energy_f64(dx, dz, ra, *dp), energy_scale_f64(dx, dz, ra, *dp)
        worst = _worst(got[:, :2], want[:, :2], scale[:, :2])
        rel = float(((got[:, 2] - want[:, 2]).abs() / want[:, 2].clamp_min(1e-300)).max())
        print(f"fractional ra, r {r} {prec}: worst |kernel - float64| / sum|terms| = {worst:.2e}, sum(ra) relative {rel:.2e}")
        assert worst <= BAR and rel <= case["S"] * 2.0 ** -53
        assert bool((got[2] == 0).all()) and bool((got[[0, 1, 3]] > 0).all())


@pytest.mark.parametrize("r,prec", [(0.5, "lean"), (0.4, "ieee"), (0.65, "lean"), (0.8, "ieee")])
def test_energy_is_the_sum_of_the_device_grids_when_no_ray_is_cut(r, prec):
    """Rays inside 0.9 of the half window, ks 21: spp E[:, :2] against the sums of forward_integral_lr's raw grids, within
    the project's forward bar of 1e-5 relative."""
    ks, ps = 21, 0.00431
    case = make_case(np.random.default_rng(int(100 * r)), 1500, 5, ks, ps, 0.78, 1.44, 0.3, r, prec)
    case["o"][..., :2] *= 0.9 / 1.25
    ray = _ray(case)
    half = (ks / 2 - 0.5) * ps
    assert float(np.abs(case["o"][..., :2]).max()) <= 0.9 * half
    dp = tuple(case[k] for k in "hfwr")
    L, R = forward_integral_lr(ray, ps, ks, pointc_ref=_t(case["cen"]), param_list=[*dp, "l"], precision=prec)
    sums = torch.stack((L.double().sum((1, 2)), R.double().sum((1, 2))), -1)
    E = dp_energy(ray, dp, prec)
    rel = float(((E[:, :2] - sums).abs() / sums).max())
    print(f"r {r} {prec}: |energy sums - sums of the raw grids| / sums = {rel:.2e}")
    assert bool((sums > 0).all()) and rel <= 1e-5


# ------------------------------------------------------------------ the backward fuzz
@pytest.mark.parametrize("seed", range(len(FUZZ_TABLE)))
def test_energy_grad_kernel_against_the_float64_restatement(seed):
    case = _fuzz(seed)
    ray, G, want = _ray(case), case["G"], case["grad"]
    S, N, M = case["S"], case["N"], case["S"] * case["N"]
    # (dh, df, dw): per point and in total
    rc, part = _abi_energy_grad(case, ray, G)
    assert rc == 0 and part.shape == (N, _slices(N, S), 3)
    per_point = part.sum(1).cpu()
    w_point = _worst(per_point, want["per_point"], want["per_point_scale"])
    w_theta = _worst(per_point.sum(0), want["theta"], want["theta_scale"])
    # the rays' terms, written (accumulate = 0) into a buffer of NaN
    rg = torch.full((4, M), float("nan"), dtype=torch.float32, device=DEV)
    rc, none = _abi_energy_grad(case, ray, G, partial=False, ray_grad=rg)
    assert rc == 0 and none is None
    assert bool((rg[:2] == 0).all()) and bool(torch.isfinite(rg).all())
    dead = case["rays"][4] == 0
    worst_ray = 0.0
    for row, key in ((2, "g_dx"), (3, "g_dz")):
        got, ref = _sn(rg[row].cpu().double(), case), want[key]
        assert bool((got[dead] == 0).all())
        top = float(ref.abs().max())
        if top == 0:
            assert not got.any()
            continue
        bar = BAR * torch.maximum(ref.abs(), torch.full_like(ref, top))
        worst_ray = max(worst_ray, float(((got - ref).abs() / bar).max()) * BAR)
        assert bool(((got - ref).abs() <= bar).all()), (key, float(((got - ref).abs() / bar).max()))
        # and summed over a point's rays, against the sum of the magnitudes
        assert _worst(got.sum(0), ref.sum(0), ref.abs().sum(0)) <= BAR
    print(f"energy grad fuzz {seed}: S {S} N {N} r {case['r']:.4f} {case['precision']}: worst |kernel - float64| / "
          f"sum|terms|: per point {w_point:.2e}, h,f,w {w_theta:.2e}; per ray / max(|term|, row max) {worst_ray:.2e}")
    assert w_point <= BAR and w_theta <= BAR
    # accumulate = 1 on a buffer the splat's backward filled: prefill + fresh, bit for bit, rows 0 and 1 left alone
    gen = torch.Generator().manual_seed(seed)
    ks = case["ks"]
    GL, GR = (torch.randn((N, ks, ks), generator=gen).to(DEV) for _ in range(2))
    pre = torch.full((4, M), float("nan"), dtype=torch.float32, device=DEV)
    dpp = _dpp(case)
    _lib.check(_lib.lib().sdirt_forward_integral_grad_rays(
        ray.c_rays(), S, N, float(case["ps"]), ks, dptr(_t(case["cen"])), C.byref(dpp), _flags(case["precision"]), dptr(GL),
        dptr(GR), None, _slices(N, S), dptr(pre), stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pre).all()) and bool(pre.any())
    buf = pre.clone()
    rc, _ = _abi_energy_grad(case, ray, G, partial=False, ray_grad=buf, accumulate=1)
    assert rc == 0 and torch.equal(buf, pre + rg) and torch.equal(buf[:2], pre[:2])
    # determinism, and the Python layer gives the sums of the C entry
    rc, part2 = _abi_energy_grad(case, ray, G)
    rg2 = torch.full_like(rg, float("nan"))
    _abi_energy_grad(case, ray, G, partial=False, ray_grad=rg2)
    assert torch.equal(part, part2) and torch.equal(rg, rg2)
    h, f, w = (torch.tensor(case[k], dtype=torch.float64, requires_grad=True) for k in "hfw")
    E = dp_energy(ray, (h, f, w, case["r"]), case["precision"])
    assert E.grad_fn is not None
    (G.to(DEV) * E).sum().backward()
    assert [float(v.grad) for v in (h, f, w)] == part.sum(1).sum(0).tolist()


def test_bad_arguments_return_a_status_before_any_launch():
    case = _kill_fragile(make_case(np.random.default_rng(11), 300, 2, 9, 0.00431, *DP[:3], 0.5, "lean"))
    ray = _ray(case)
    lib = _lib.lib()
    ns = _slices(2, 300)
    G = torch.ones((2, 3), dtype=torch.float64)
    bad_dp = [("r = 0", _lib.DpParams(*DP[:3], 0.0), "dp->r"), ("f == h", _lib.DpParams(0.78, 0.78, 0.3, 0.5), "dp->f"),
              ("NULL dp", None, "null dp")]
    for name, kw, text in [("n_slices + 1", dict(n_slices=ns + 1), "n_slices"), ("n_slices - 1", dict(n_slices=ns - 1), "n_slices")] + \
            [(n, dict(dp=d, n_slices=ns), t) for n, d, t in bad_dp]:
        rc, partial = _abi_energy(case, ray, fill=-7.0, **kw)
        msg = lib.sdirt_last_error().decode()
        assert rc == -1 and text in msg, (name, rc, msg)                       # SDIRT_ERR_INVALID_ARGUMENT
        assert bool((partial == -7.0).all()), name
        rg = torch.full((4, 600), -7.0, dtype=torch.float32, device=DEV)
        rc, part = _abi_energy_grad(case, ray, G, ray_grad=rg, fill=-7.0, **kw)
        msg = lib.sdirt_last_error().decode()
        assert rc == -1 and text in msg, (name, rc, msg)
        assert bool((part == -7.0).all()) and bool((rg == -7.0).all()), name
    rc, part = _abi_energy_grad(case, ray, G, partial=False, ray_grad=None)     # both outputs NULL
    assert rc == -1 and "both null" in lib.sdirt_last_error().decode()
    st = stream_ptr(torch.device(DEV))
    dpp = _dpp(case)
    assert lib.sdirt_dp_energy(ray.c_rays(), 300, 2, C.byref(dpp), 0, None, ns, st) == -1           # no output at all
    # N = 0: SDIRT_OK and nothing written, whatever n_slices says
    out = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
    assert lib.sdirt_dp_energy(ray.c_rays(), 300, 0, C.byref(dpp), 0, dptr(out), 0, st) == 0
    assert lib.sdirt_dp_energy_grad(ray.c_rays(), 300, 0, C.byref(dpp), 0, dptr(out), dptr(out), 0, None, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # and the call they all deviate from
    rc, partial = _abi_energy(case, ray, fill=-7.0, n_slices=ns)
    flat, n = partial.reshape(-1), 2 * ns * 3
    assert rc == 0 and bool((flat[:n] != -7.0).all()) and bool((flat[n:] == -7.0).all())


# ------------------------------------------------------------------ on rf50mm
PTS = [[0.0, 0.0, -1500.0], [0.98, 0.98, -1500.0], [-0.98, 0.98, -1500.0], [0.35, -0.2, -1200.0], [-0.35, -0.2, -1200.0],
       [0.6, 0.45, -2500.0], [-0.6, 0.45, -2500.0], [0.0, 0.9, -400.0]]
MIRRORS = [(1, 2), (3, 4), (5, 6)]               # (x, y, z) and (-x, y, z)


@pytest.fixture(scope="module")
def lens():
    return make_lens("rf50mm", DEV, load_state("rf50mm"))


@pytest.fixture(scope="module")
def pupil(lens):
    """Fixed pupil samples (primary, chief ray), as a psf call draws them."""
    torch.manual_seed(27)
    with torch.no_grad():
        lens.psf_lr(torch.tensor(PTS[:2]), ks=21, spp=SPP)
    x2, y2, xc, yc = (t.clone() for t in lens.last_pupil_points)
    assert x2.numel() == SPP
    return (x2, y2), (xc, yc)


class _Bundles:
    """Keeps the sensor-plane bundle (and, of a recording call, the TraceRecord) of the staged calls made inside the block."""

    def __init__(self, lens):
        self.lens, self.rays, self.records = lens, [], []

    def __enter__(self):
        inner = self.lens._staged_rays

        def wrapped(*args, **kwargs):
            out = inner(*args, **kwargs)
            self.rays.append(out[0])
            if len(out) > 2:
                self.records.append(out[2])
            return out
        self.lens._staged_rays = wrapped
        return self

    def __exit__(self, *exc):
        del self.lens.__dict__["_staged_rays"]


def test_psf_lr_energy_is_the_entry_on_the_calls_own_bundle(lens, pupil):
    pts = torch.tensor(PTS)
    N, kw = len(PTS), dict(ks=21, dp=DP, pupil_xy=pupil[0], center_pupil_xy=pupil[1])
    with torch.no_grad(), _Bundles(lens) as cap:
        L, R, E = lens.psf_lr(pts, energy=True, **kw)
    (ray,) = cap.rays
    assert ray.shape == (SPP, N) and E.shape == (N, 3) and E.dtype == torch.float64
    assert torch.equal(E, dp_energy(ray, DP) / SPP)
    ra = ray.soa[6, :SPP * N].reshape(N, SPP)
    assert bool(((ra == 0) | (ra == 1)).all())
    assert torch.equal(E[:, 2], (ra == 1).double().sum(1) / SPP)                  # T: the share of the rays that arrive
    T = E[:, 2].cpu()
    assert float(T[0]) > 0.5 and float(T[1]) < float(T[0])                        # the corner is vignetted
    # L and R are the staged chain's.  Under autograd every call takes that chain, and below REPEATABLE_SPP its grids
    # (float64 tiles in LDS, rounded once) repeat bit for bit: with and without the energy, the same bits
    h = torch.tensor(DP[0], requires_grad=True)
    Lg, Rg = lens.psf_lr(pts, **dict(kw, dp=(h, *DP[1:])))
    Le, Re, Ee = lens.psf_lr(pts, energy=True, **dict(kw, dp=(h, *DP[1:])))
    assert torch.equal(Lg.detach(), Le.detach()) and torch.equal(Rg.detach(), Re.detach()) and torch.equal(Ee.detach(), E)
    # At a ks the fused kernel does not take, the call without the energy is the staged chain too.  There the splat adds
    # into the grids in HBM with float atomics, whose order is not fixed: a sum of three or more terms may round
    # differently from one call to the next, a sum of two may not (fp32 addition commutes).  Two samples per point: at
    # most two rays meet in a pixel, so the grids are the same bits whatever the order.
    big = dict(kw, ks=_lib.MAX_KS + 2)
    two = dict(big, pupil_xy=(pupil[0][0][:2].clone(), pupil[0][1][:2].clone()))
    with torch.no_grad():
        L0, R0 = lens.psf_lr(pts, **two)
        L1, R1, E1 = lens.psf_lr(pts, energy=True, **two)
    assert float(L0.max()) > 0 and E1.shape == (N, 3)
    assert torch.equal(L0, L1) and torch.equal(R0, R1)
    # All 960 samples: a pixel's sum of n <= 4 SPP positive fp32 terms (four taps per ray) differs between two orders by at
    # most n 2^-24 of itself, and each grid is divided by its own maximum, which moves alike: 2 n 2^-24 of the peak, 1
    with torch.no_grad():
        L0, R0 = lens.psf_lr(pts, **big)
        L0b, R0b = lens.psf_lr(pts, **big)
        L1, R1, E1 = lens.psf_lr(pts, energy=True, **big)
    spread = max(float((L0 - L1).abs().max()), float((R0 - R1).abs().max()))
    print(f"ks {big['ks']}, spp {SPP}: two calls without the energy bit-equal: {torch.equal(L0, L0b) and torch.equal(R0, R0b)}; "
          f"with against without the energy: max |difference| = {spread:.2e} of the peak")
    assert spread <= 2 * 4 * SPP * 2.0 ** -24 and torch.equal(E1, E)
    assert L.shape == (N, 21, 21) and float(L.max()) == pytest.approx(1.0, abs=1e-5)
    # one point: [3]
    with torch.no_grad():
        l1, r1, e1 = lens.psf_lr(pts[3], energy=True, **kw)
    assert l1.shape == (21, 21) and e1.shape == (3,)
    with pytest.raises(ValueError):
        lens.psf_lr(pts, energy=True, defer=True, **kw)
    with pytest.raises(ValueError):
        lens.psf_lr(pts, energy=True, _default_r_zero=True, **kw)
    with torch.no_grad():                                                         # energy=False: as before, a pair
        assert len(lens.psf_lr(pts, **kw)) == 2
    on_axis, corner = E[0].cpu(), E[1].cpu()
    print(f"rf50mm, ks 21, spp {SPP}: E_L / E_R on axis {float(on_axis[0] / on_axis[1]):.4f} (T {float(on_axis[2]):.3f}), at the "
          f"field corner (0.98, 0.98) {float(corner[0] / corner[1]):.4f} (T {float(corner[2]):.3f}), at (-0.98, 0.98) "
          f"{float(E[2, 0] / E[2, 1]):.4f}")


def test_mirrored_points_swap_left_and_right_energy(lens, pupil):
    """(x, y, z) with pupil samples (x2, y2) against (-x, y, z) with (-x2, y2): the lens is rotationally symmetric, the
    formulas satisfy d_l(t) = d_r(-t) and negation is exact, so E_L of one is E_R of the other, within the forward bar."""
    pts = torch.tensor(PTS)
    (x2, y2), (xc, yc) = pupil
    with torch.no_grad():
        _, _, E = lens.psf_lr(pts, ks=21, dp=DP, pupil_xy=(x2, y2), center_pupil_xy=(xc, yc), energy=True)
        _, _, Em = lens.psf_lr(pts, ks=21, dp=DP, pupil_xy=(-x2, y2), center_pupil_xy=(-xc, yc), energy=True)
    E, Em = E.cpu(), Em.cpu()
    worst = 0.0
    for a, b in MIRRORS + [(b, a) for a, b in MIRRORS] + [(0, 0), (7, 7)]:
        rel = max(abs(float(E[a, 0] - Em[b, 1])) / float(Em[b, 1]), abs(float(E[a, 1] - Em[b, 0])) / float(Em[b, 0]))
        worst = max(worst, rel)
        assert float(E[a, 2]) == float(Em[b, 2])                                  # the same rays arrive
    print(f"mirror: worst |E_L(x) - E_R(-x)| / E_R = {worst:.2e}")
    assert worst <= 1e-5
    assert abs(float(E[1, 0] / E[1, 1]) - 1.0) > 1e-3                             # and off axis there is shading to swap


def _energy_ray_grad(rec, ge):
    ray = rec.ray
    S, N = ray.shape
    rg = torch.full((4, S * N), float("nan"), dtype=torch.float32, device=DEV)
    dpp = _lib.DpParams(*DP)
    _lib.check(_lib.lib().sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dpp), _flags(rec.precision), dptr(ge), None,
                                               _slices(N, S), dptr(rg), 0, stream_ptr(torch.device(DEV))))
    return rg


def test_energy_only_loss_reaches_the_surfaces_through_the_recorded_trace(lens, pupil):
    pts = torch.tensor(PTS)
    N = len(PTS)
    G = torch.randn((N, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(DEV)
    theta = lens.surface_parameters().requires_grad_()
    with _Bundles(lens) as cap:
        L, R, E = lens.psf_lr(pts, ks=21, dp=DP, pupil_xy=pupil[0], center_pupil_xy=pupil[1], surface_params=theta, energy=True)
    (G * E).sum().backward()
    (rec,) = cap.records
    rg = _energy_ray_grad(rec, (G / SPP).contiguous())
    want = _abi(rec, rg, "sdirt_trace2sensor_grad").sum(0)[:, :N_COLUMNS].to(torch.float32).cpu()
    assert float(theta.grad.abs().max()) > 0 and torch.equal(theta.grad, want)


def test_energy_only_loss_reaches_the_glass_through_the_eta_entry(lens, pupil):
    pts = torch.tensor(PTS)
    N = len(PTS)
    G = torch.randn((N, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(6)).to(DEV)
    glass = lens.glass_parameters().requires_grad_()
    with _Bundles(lens) as cap:
        L, R, E = lens.psf_lr(pts, ks=21, dp=DP, pupil_xy=pupil[0], center_pupil_xy=pupil[1], glass_params=glass, energy=True)
    (G * E).sum().backward()
    (rec,) = cap.records
    rg = _energy_ray_grad(rec, (G / SPP).contiguous())
    g_eta = _abi(rec, rg, "sdirt_trace2sensor_grad_eta").sum(0)[:, N_COLUMNS]
    again = lens.glass_parameters().requires_grad_()
    eta = lens._glass_eta(again, DEFAULT_WAVE)
    eta.backward(g_eta.to(device=eta.device, dtype=eta.dtype))
    own = torch.as_tensor(lens.glass_owned())
    assert float(glass.grad[own].abs().max()) > 0 and torch.equal(glass.grad, again.grad)
    assert bool((glass.grad[~own] == 0).all())


def test_a_loss_on_grids_and_energy_is_the_sum_of_the_separate_gradients(lens, pupil):
    """theta and h from a loss on L, R and E together against the sum of the gradients of the three losses taken one by
    one: the kernels are deterministic and the energy's ray terms are rounded to fp32 before they join the splat's, so
    the difference is fp32 rounding of the sums: 2^-23 of the magnitudes (the rule of
    test_psf_rgb_gradient_is_the_sum_of_its_wavelengths).  One column is no sum of magnitudes at all: the stop's d moves a
    plane that does not refract along the ray, its terms vanish identically and every walk returns the float64 rounding
    of the terms it cancels from, n_rays 2^-53 of the size of the column's other sums (the floor of
    test_gpu_trace_grad._check_against_restatement); that much is allowed on top."""
    pts = torch.tensor(PTS)
    N, ks = len(PTS), 21
    gen = torch.Generator().manual_seed(7)
    GL, GR = (torch.randn((N, ks, ks), generator=gen).to(DEV) for _ in range(2))
    GE = (10.0 * torch.randn((N, 3), dtype=torch.float64, generator=gen)).to(DEV)

    def run(use):
        theta = lens.surface_parameters().requires_grad_()
        h = torch.tensor(DP[0], requires_grad=True)
        L, R, E = lens.psf_lr(pts, ks=ks, dp=(h, *DP[1:]), pupil_xy=pupil[0], center_pupil_xy=pupil[1], surface_params=theta,
                              energy=True)
        terms = {"L": (GL * L).sum().double(), "R": (GR * R).sum().double(), "E": (GE * E).sum()}
        sum(terms[k] for k in use).backward()
        return theta.grad.double(), h.grad.double().reshape(1)
    both_t, both_h = run("LRE")
    parts = [run(k) for k in "LRE"]
    for name, both, terms in (("theta", both_t, [p[0] for p in parts]), ("h", both_h, [p[1] for p in parts])):
        total, mag = sum(terms), sum(t.abs() for t in terms)
        assert all(float(t.abs().max()) > 0 for t in terms)
        floor = N * SPP * 2.0 ** -53 * mag.reshape(-1, mag.shape[-1]).max(0).values
        diff = (both - total).abs()
        err = float((diff / (mag + 2.0 ** 23 * floor).clamp_min(1e-300)).max())
        print(f"{name}: max |joint - sum of the three| / (sum|terms| + floor) = {err:.3e}")
        if name == "theta":
            stop = lens.aper_idx
            print(f"the stop's d: joint {float(both[stop, 0]):.3e}, separate {[float(t[stop, 0]) for t in terms]}, the column's "
                  f"largest magnitude {float(mag[:, 0].max()):.3e}")
        assert bool((diff <= 2.0 ** -23 * mag + floor).all())


def test_the_sensor_position_gets_exactly_nothing_from_the_energy(lens, pupil):
    pts = torch.tensor(PTS)
    G = torch.randn((len(PTS), 3), dtype=torch.float64, generator=torch.Generator().manual_seed(8)).to(DEV)
    d = torch.tensor(float(lens.d_sensor), requires_grad=True)
    h = torch.tensor(DP[0], requires_grad=True)
    L, R, E = lens.psf_lr(pts, ks=21, dp=(h, *DP[1:]), pupil_xy=pupil[0], center_pupil_xy=pupil[1], d_sensor=d, energy=True)
    (G * E).sum().backward()
    assert d.grad is not None and float(d.grad) == 0.0
    assert h.grad is not None and float(h.grad) != 0.0
    d2 = torch.tensor(float(lens.d_sensor), requires_grad=True)              # while the grids do move with the sensor
    L, R, E = lens.psf_lr(pts, ks=21, dp=DP, pupil_xy=pupil[0], center_pupil_xy=pupil[1], d_sensor=d2, energy=True)
    ((L * L).sum() + (G * E).sum()).backward()
    assert float(d2.grad) != 0.0


# ------------------------------------------------------------------ the volume
def test_photometric_volume_carries_its_energy_into_the_render(lens, pupil):
    """psf_volume(photometric=True) on a 3 x 3 x 2 grid with h requiring a gradient, rendered on a 16 x 24 image.  h.grad
    of an L2 image loss against the same graph built by hand (psf_lr(energy=True) + photometric_scale +
    local_dp_psf_render_volume): within 2 max(s, 1e-4) relative, s the hand-built path's own spread, fp32 render stage
    against the same graph with that stage's gradient from the float64 restatement."""
    from render_volume_f64 import render_volume_f64
    H, W, ks, C_ = 16, 24, 21, 3
    gen = torch.Generator().manual_seed(9)
    img = torch.rand((1, C_, H, W), generator=gen).to(DEV)
    z = torch.rand((1, H, W), generator=gen).to(DEV)
    kw = dict(grid=(3, 3), z=2, ks=ks, spp=SPP, pupil_xy=pupil[0], center_pupil_xy=pupil[1])
    with torch.no_grad():
        target = torch.roll(lens.psf_volume(dp=(0.70, *DP[1:]), photometric=True, **kw).render(img, z), 1, -1)
        assert lens.psf_volume(dp=DP, **kw).energy is None
    # photometric=False, along the same path (h requires a gradient: the staged chain under autograd): as today
    plain = lens.psf_volume(dp=(torch.tensor(DP[0], requires_grad=True), *DP[1:]), **kw)
    assert plain.energy is None and plain.psf.grad_fn is not None
    assert float((plain.psf.detach().sum((-1, -2)) - 1).abs().max()) <= 1e-5
    h = torch.tensor(DP[0], requires_grad=True)
    vol = lens.psf_volume(dp=(h, *DP[1:]), photometric=True, **kw)
    assert vol.psf.shape == (2, 3, 3, 2, ks, ks) and vol.energy.shape == (2, 3, 3, 3) and vol.energy.dtype == torch.float64
    E = vol.energy.detach()
    gain = E[..., :2] / E[..., :2].mean()
    sums = vol.psf.detach().double().sum((-1, -2))
    print(f"volume: kernel sums from {float(sums.min()):.4f} to {float(sums.max()):.4f}, mean {float(sums.mean()):.6f}; "
          f"worst |sum - E / mean(E)| = {float((sums - gain).abs().max()):.2e}")
    assert float((sums - gain).abs().max()) <= 1e-5 and abs(float(sums.mean()) - 1) <= 1e-5
    assert float(sums.max() - sums.min()) > 1e-3                                # there is shading to render
    out = vol.render(img, z)
    with torch.no_grad():
        by_hand = local_dp_psf_render_volume(img, photometric_scale(plain.psf.detach(), E), vol.x_nodes, vol.y_nodes, vol.z_nodes, z, ks)
    assert torch.equal(out.detach(), by_hand)
    loss = ((out - target) ** 2).sum()
    loss.backward()
    g_fused = float(h.grad)
    # the same graph by hand
    h2 = torch.tensor(DP[0], requires_grad=True)
    L, R, E2 = lens.psf_lr(vol.points(), ks=ks, dp=(h2, *DP[1:]), pupil_xy=pupil[0], center_pupil_xy=pupil[1], energy=True)
    psf = torch.stack((L, R), -3)
    psf = (psf / psf.sum((-1, -2), keepdim=True).clamp_min(1e-30)).reshape(2, 3, 3, 2, ks, ks)
    psf = photometric_scale(psf, E2.reshape(2, 3, 3, 3))
    out2 = local_dp_psf_render_volume(img, psf, vol.x_nodes, vol.y_nodes, vol.z_nodes, z, ks)
    tables = volume_segment_tables(vol.x_nodes, vol.y_nodes, vol.z_nodes, z, H, W)
    v64 = psf.detach().cpu().double().requires_grad_(True)
    l64, r64 = render_volume_f64(img.cpu(), v64, tuple(t.cpu() for t in tables), ks)
    ((torch.cat([l64, r64], 1) - target.cpu().double()) ** 2).sum().backward()
    (g_f64,) = torch.autograd.grad(psf, h2, grad_outputs=v64.grad.float().to(DEV), retain_graph=True)
    ((out2 - target) ** 2).sum().backward()
    g_hand, g_f64 = float(h2.grad), float(g_f64)
    s = abs(g_hand - g_f64) / abs(g_f64)
    rel = abs(g_fused - g_hand) / abs(g_hand)
    print(f"d loss / d h: psf_volume(photometric=True) {g_fused:.9e}, by hand {g_hand:.9e}, by hand with the float64 render "
          f"gradient {g_f64:.9e}; spread s = {s:.3e}, |volume - by hand| / |by hand| = {rel:.3e}, allowed {2 * max(s, 1e-4):.3e}")
    assert np.isfinite(g_fused) and g_fused != 0.0
    assert rel <= 2 * max(s, 1e-4)
