"""Gradients of dual-pixel PSFs on the GPU: psf_diff / psf_lr / psf_rgb / forward_integral differentiable in the DP
sensor parameters (h, f, w) and, with center=False, in the points; the backward kernel sdirt_forward_integral_grad
against the float64 restatement (tests/splat_f64.py), which tests/test_dp_grad_cpu.py holds against the reference's own
autograd.

The backward fuzz and its edge cases run on synthetic sensor-plane rays (fuzz_case: every stack geometry, both
models, every launch shape); the rays a float64 reference cannot judge (splat_f64.fragile_rays) are killed before
either side sees them.  fuzz_case needs no GPU: tests/test_dp_grad_cpu.py checks on every machine that the default
seeds reach both states of every clamp gate and stay under the fragile-ray cap."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import load_state, make_lens
from splat_f64 import boundaries, fragile_rays, gate_states, live_in_window, max_normalise, splat_f64

from sdirt_amd import _lib
from sdirt_amd.basics import dptr, stream_ptr
from sdirt_amd.monte_carlo import forward_integral_lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = (0.78, 1.44, 0.3)


@pytest.fixture(scope="module")
def lens():
    return make_lens("rf50mm", DEV, load_state("rf50mm"))


def _leaves(vals=DP, dtype=torch.float32):
    return [torch.tensor(v, dtype=dtype, requires_grad=True) for v in vals]


PTS = [[0.0, 0.0, -1500.0], [0.35, -0.2, -1200.0], [-0.6, 0.45, -2500.0]]


def _case(lens, spp=1024, seed=27):
    """Fixed pupil samples (primary, chief ray) for PTS, as a psf call draws them, and an upstream weight."""
    torch.manual_seed(seed)
    with torch.no_grad():
        lens.psf_lr(torch.tensor(PTS), ks=21, spp=spp)
    x2, y2, xc, yc = (t.clone() for t in lens.last_pupil_points)
    G = torch.randn((len(PTS), 21, 21), generator=torch.Generator().manual_seed(seed)).to(DEV)
    return torch.tensor(PTS), (x2, y2), (xc, yc), G


def test_psf_diff_backward_sets_finite_grads(lens):
    h, f, w = _leaves()
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.3, -0.2, -1200.0]])
    psf = lens.psf_diff(pts, ks=31, spp=2048, param_list=[h, f, w, 0.5, "l"])
    assert psf.grad_fn is not None
    (psf * torch.linspace(-1, 1, psf.numel(), device=psf.device).reshape(psf.shape)).sum().backward()
    for t in (h, f, w):
        assert t.grad is not None and torch.isfinite(t.grad) and float(t.grad) != 0.0


def _staged(lens, pts, spp, center):
    """The staged chain's own sensor-plane rays and centres for `pts`."""
    N = pts.shape[0]
    with torch.no_grad():
        po = lens._points_to_object(pts)
        cen = torch.empty((N, 2), dtype=torch.float32, device=DEV)
        ray, spp = lens._staged_rays(pts, po, N, 0.589, spp, center, None, None, cen)
    soa = ray.soa[:, :spp * N].view(7, N, spp).transpose(1, 2)          # point-major -> [7, S, N]
    return ray, cen, [soa[k].cpu() for k in (0, 1, 3, 5, 6)]


@pytest.mark.parametrize("r,ks,prec,center", [
    (0.5, 21, "lean", True), (0.65, 21, "ieee", False), (0.5, 65, "ieee", False), (0.65, 65, "lean", True),
    (0.5, 150, "lean", False), (0.65, 150, "ieee", True)])
def test_kernel_matches_float64_restatement_on_its_own_rays(lens, r, ks, prec, center):
    assert ks in (21, 65) or ks > _lib.MAX_KS
    torch.manual_seed(7)
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.4, -0.3, -1200.0], [-0.7, 0.5, -2500.0]])
    S, N = 2048, pts.shape[0]
    ray, cen, rays = _staged(lens, pts, S, center)
    gen = torch.Generator().manual_seed(ks)
    GL, GR = torch.randn((N, ks, ks), generator=gen), torch.randn((N, ks, ks), generator=gen)
    # the kernel: forward_integral_lr with h, f, w and pointc_ref requiring grad
    h, f, w = _leaves()
    c = cen.clone().requires_grad_(True)
    L, R = forward_integral_lr(ray, lens.pixel_size, ks, pointc_ref=c, param_list=[h, f, w, r, "l"], precision=prec)
    ((GL.to(DEV) * L).sum() + (GR.to(DEV) * R).sum()).backward()
    got = np.array([float(h.grad), float(f.grad), float(w.grad)] + c.grad.cpu().numpy().ravel().tolist())
    # the restatement with per-ray leaves: the sum of their gradients is the gradient, the sum of |.| the scale
    hv, fv, wv = (torch.full((S, N), v, dtype=torch.float64, requires_grad=True) for v in DP)
    cv = cen.cpu().double().unsqueeze(0).expand(S, N, 2).clone().requires_grad_(True)
    L6, R6 = splat_f64(*rays, cv, lens.pixel_size, ks, hv, fv, wv, float(np.float32(r)))
    ((GL.double() * L6).sum() + (GR.double() * R6).sum()).backward()
    want = np.array([float(t.grad.sum()) for t in (hv, fv, wv)] + cv.grad.sum(0).numpy().ravel().tolist())
    scale = np.array([float(t.grad.abs().sum()) for t in (hv, fv, wv)] + cv.grad.abs().sum(0).numpy().ravel().tolist())
    assert np.all(scale > 0)
    assert np.all(np.abs(got - want) <= 1e-5 * scale), (got, want, np.abs(got - want) / scale)
    # the forward is the kernel's raw grids
    assert np.abs(L.detach().cpu().numpy() - L6.detach().numpy()).max() <= 1e-5 * float(L6.detach().abs().max())


@pytest.mark.parametrize("ks", [31, 65])
def test_psf_under_grad_agrees_with_no_grad_call(lens, ks):
    pts, pxy, cxy, _ = _case(lens)
    h, f, w = _leaves()
    Lg, Rg = lens.psf_lr(pts, ks=ks, dp=(h, f, w, 0.5), pupil_xy=pxy, center_pupil_xy=cxy)
    L0, R0 = lens.psf_lr(pts, ks=ks, dp=(*DP, 0.5), pupil_xy=pxy, center_pupil_xy=cxy)
    for a, b in ((Lg, L0), (Rg, R0)):
        d = float((a.detach() - b).abs().max())
        print(f"ks {ks}: |PSF under grad - no-grad PSF| = {d:.2e} (bit-equal: {torch.equal(a.detach(), b)})")
        assert d <= 1e-6 * float(b.abs().max())


def test_two_backward_passes_are_bit_identical(lens):
    pts, pxy, cxy, G = _case(lens)
    out = []
    for _ in range(2):
        h, f, w = _leaves()
        L, R = lens.psf_lr(pts, ks=21, dp=(h, f, w, 0.65), pupil_xy=pxy, center_pupil_xy=cxy)
        ((G * L).sum() + (G * R).sum()).backward()
        out.append([t.grad.item() for t in (h, f, w)])
    assert out[0] == out[1]


def test_psf_rgb_gradient_is_the_sum_of_its_three_psf_calls(lens):
    pts, pxy, cxy, _ = _case(lens)
    ks = 21
    P = torch.stack([torch.stack([pxy[0]] * 3), torch.stack([pxy[1]] * 3)])          # [2, 3, spp]
    Pc = torch.stack([torch.stack([cxy[0]] * 3), torch.stack([cxy[1]] * 3)])
    G = torch.randn((pts.shape[0], 3, ks, ks), generator=torch.Generator().manual_seed(3)).to(DEV)
    h, f, w = _leaves()
    rgb = lens.psf_rgb(pts, ks=ks, param_list=[h, f, w, 0.5, "r"], pupil_xy=P, center_pupil_xy=Pc)
    (G * rgb).sum().backward()
    got = [t.grad.item() for t in (h, f, w)]
    want = np.zeros(3)
    from sdirt_amd.basics import WAVE_RGB
    for k, wv in enumerate(WAVE_RGB):
        h2, f2, w2 = _leaves()
        _, R = lens.psf_lr(pts, ks=ks, wvln=wv, dp=(h2, f2, w2, 0.5), pupil_xy=(P[0][k], P[1][k]),
                           center_pupil_xy=(Pc[0][k], Pc[1][k]))
        (G[:, k] * R).sum().backward()
        want += [t.grad.item() for t in (h2, f2, w2)]
    np.testing.assert_allclose(got, want, rtol=1e-6)
    with torch.no_grad():                                   # and the values are the fused call's
        ref = lens.psf_rgb(pts, ks=ks, param_list=[*DP, 0.5, "r"], pupil_xy=P, center_pupil_xy=Pc)
    assert float((rgb.detach() - ref).abs().max()) <= 1e-6


def _fit(lens, start, free, target_dp, steps, lr):
    pts, pxy, cxy, _ = _case(lens)
    ks = 21
    with torch.no_grad():
        tL, tR = lens.psf_lr(pts, ks=ks, dp=(*target_dp, 0.5), pupil_xy=pxy, center_pupil_xy=cxy)
    params = [torch.tensor(v, requires_grad=k in free) for k, v in enumerate(start)]
    opt = torch.optim.Adam([params[k] for k in free], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 - s / steps)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        L, R = lens.psf_lr(pts, ks=ks, dp=(*params, 0.5), pupil_xy=pxy, center_pupil_xy=cxy)
        loss = ((L - tL) ** 2).sum() + ((R - tR) ** 2).sum()
        loss.backward()
        losses.append(loss.item())
        opt.step()
        sched.step()
    return [p.item() for p in params], losses


def test_fit_recovers_w(lens):
    (h, f, w), losses = _fit(lens, (0.78, 1.44, 0.25), [2], (0.78, 1.44, 0.30), steps=100, lr=4e-3)
    print(f"w fit: {w:.5f} after 100 steps, loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert abs(w - 0.30) < 1e-3


def test_joint_fit_reduces_the_loss(lens):
    p, losses = _fit(lens, (0.76, 1.47, 0.27), [0, 1, 2], (0.78, 1.44, 0.30), steps=100, lr=3e-3)
    print(f"joint fit: (h, f, w) = {p}, loss {losses[0]:.3e} -> {min(losses):.3e}")
    assert min(losses) <= losses[0] / 100


# ------------------------------------------------------------------ the backward fuzz: synthetic rays, every geometry
# seed -> ((S, N), ks, third of r): one slice and several, a short last slice, S below a workgroup, N in the
# thousands; ks on both sides of the LDS staging switch (78 | 79, each with r on both sides of 0.5), even, 2, and
# above the forward's LDS limit
FUZZ_TABLE = [((1500, 5), 21, 0), ((257, 1), 78, 1), ((4100, 3), 150, 2), ((63, 5), 79, 0), ((5000, 1), 65, 1),
              ((40, 3000), 9, 2), ((2048, 40), 78, 0), ((1500, 5), 79, 1), ((2048, 40), 2, 2), ((1, 5), 22, 0),
              ((40, 3000), 22, 1), ((4100, 3), 2, 0)]
R_THIRDS = [(0.15, 0.5), (0.5, 0.70), (0.71, 0.95)]      # gi closes below 0.5; the u gate closes only below 0.707
SPARSE_FORWARD_BAR = {2}    # entries of FUZZ_TABLE whose forward check is widened to 2 ks 2^-23: see the fuzz's docstring
FUZZ_SEED0 = 2700
FRAGILE_CAP = 0.005         # of the live in-window rays of a case; 2 rays where a case has fewer than 400
FEW_RAYS = 400


def _f32(v):
    return float(np.float32(v))


def make_case(rng, S, N, ks, ps, h, f, w, r, precision="lean", dead=0.15, x_tan=None, kill_fragile=True,
              weights=False):
    """Synthetic sensor-plane rays as the kernels read them, no GPU involved: positions uniform in +-1.25 x the half
    window, directions N(0, 0.2) normalised (or d = (-x_tan, 0, 1) normalised), `dead` of them with ra = 0, centres
    within half a pixel of 0 (weights: the live rays' ra uniform in [0.25, 1) instead of 1).  The rays
    fragile_rays flags get ra = 0 HERE, before the kernel or the restatement sees them.  h, f, w, r are rounded to
    fp32 (the leaves are fp32 tensors)."""
    h, f, w, r = (_f32(v) for v in (h, f, w, r))
    half = (ks / 2 - 0.5) * ps
    o = np.zeros((S, N, 3), np.float32)
    o[..., :2] = rng.uniform(-1.25 * half, 1.25 * half, (S, N, 2))
    o[..., 2] = 62.25
    if x_tan is None:
        d = rng.normal(0, 0.2, (S, N, 3))
        d[..., 2] = 1.0
    else:
        d = np.stack(np.broadcast_arrays(-np.asarray(x_tan, np.float64).reshape(S, N), 0.0, 1.0), -1)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    ra = (rng.random((S, N)) >= dead).astype(np.float32)
    if weights:
        ra *= rng.uniform(0.25, 1.0, (S, N)).astype(np.float32)
    cen = ((rng.random((N, 2)) - 0.5) * ps).astype(np.float32)
    rays = [torch.from_numpy(np.ascontiguousarray(a)) for a in (o[..., 0], o[..., 1], d[..., 0], d[..., 2], ra)]
    frag = fragile_rays(*rays, torch.from_numpy(cen), ps, ks, h, f, w, r)
    n_live = int(live_in_window(rays[0], rays[1], rays[4], torch.from_numpy(cen), ps, ks).sum())
    if kill_fragile:
        ra[frag.numpy()] = 0.0
    rays[4] = torch.from_numpy(ra)
    return dict(S=S, N=N, ks=ks, ps=ps, h=h, f=f, w=w, r=r, precision=precision, o=o, d=d, ra=ra, cen=cen, rays=rays,
                n_live=n_live, n_fragile=int(frag.sum()))


def fuzz_case(seed):
    (S, N), ks, third = FUZZ_TABLE[seed % len(FUZZ_TABLE)]
    rng = np.random.default_rng(FUZZ_SEED0 + seed)
    h = rng.uniform(0.4, 1.1)
    f = h + rng.uniform(0.3, 1.2)
    w = rng.uniform(0.1, 0.6)
    lo, hi = R_THIRDS[third]
    r = hi - (hi - lo) * rng.random() if third == 1 else rng.uniform(lo, hi)      # (0.5, 0.70]: never 0.5 itself
    ps = [0.046875, 0.00431][seed % 2]
    case = make_case(rng, S, N, ks, ps, h, f, w, r, precision=["lean", "ieee"][seed % 2])
    assert (case["r"] > 0.5) == (third > 0)
    return case


def fragile_within_cap(case):
    return case["n_fragile"] <= (2 if case["n_live"] < FEW_RAYS else FRAGILE_CAP * case["n_live"])


def gate_shares(case):
    """name -> (share open, share closed) of the (live in-window ray, boundary) pairs, from float64 quantities."""
    ox, oy, dx, dz, ra = case["rays"]
    live = live_in_window(ox, oy, ra, torch.from_numpy(case["cen"]), case["ps"], case["ks"])
    t = (-dx.double() / dz.double())[live]
    if t.numel() == 0:
        return {}
    return {k: (float(a.double().mean()), float(b.double().mean()))
            for k, (a, b) in gate_states(t, case["h"], case["f"], case["w"], case["r"]).items()}


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _ray(case):
    from test_gpu_parity import rays_from_fixture
    ray = rays_from_fixture(case["o"], case["d"])
    ray.ra = _t(case["ra"])
    return ray


def _upstreams(case, seed):
    gen = torch.Generator().manual_seed(seed)
    shape = (case["N"], case["ks"], case["ks"])
    return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)


def _kernel(case, GL, GR, param_list="dp"):
    """(h, f, w gradients [3], centre gradients [N, 2], L, R) of (GL . L).sum() + (GR . R).sum() through
    forward_integral_lr with h, f, w and pointc_ref requiring grad."""
    h, f, w = _leaves((case["h"], case["f"], case["w"]))
    c = _t(case["cen"]).requires_grad_(True)
    pl = [h, f, w, case["r"], "l"] if param_list == "dp" else None
    L, R = forward_integral_lr(_ray(case), case["ps"], case["ks"], pointc_ref=c, param_list=pl,
                               precision=case["precision"])
    ((GL.to(DEV) * L).sum() + (GR.to(DEV) * R).sum()).backward()
    theta = np.array([float(v.grad) if v.grad is not None else 0.0 for v in (h, f, w)])
    return theta, c.grad.cpu().numpy().astype(np.float64), L.detach().cpu().double(), R.detach().cpu().double()


def _restatement(case, GL, GR, frac_dtype=None):
    """The same from splat_f64 with per-ray leaves: (want, scale) for (h, f, w) [3] and the centres [N, 2], and
    L, R.  The sum of the per-ray gradients is the gradient, the sum of their magnitudes the scale."""
    S, N = case["S"], case["N"]
    if frac_dtype is None:
        frac_dtype = torch.float32 if case["n_live"] < FEW_RAYS else torch.float64
    hv, fv, wv = (torch.full((S, N), case[k], dtype=torch.float64, requires_grad=True) for k in "hfw")
    cv = torch.from_numpy(case["cen"]).double().unsqueeze(0).expand(S, N, 2).clone().requires_grad_(True)
    L6, R6 = splat_f64(*case["rays"], cv, case["ps"], case["ks"], hv, fv, wv, case["r"], frac_dtype=frac_dtype)
    loss = (GL.double() * L6).sum() + (GR.double() * R6).sum() if GR is not None else (GL.double() * L6).sum()
    loss.backward()
    zero = torch.zeros((S, N), dtype=torch.float64)
    g = [v.grad if v.grad is not None else zero for v in (hv, fv, wv)]
    want = (np.array([float(v.sum()) for v in g]), cv.grad.sum(0).numpy())
    scale = (np.array([float(v.abs().sum()) for v in g]), cv.grad.abs().sum(0).numpy())
    return want, scale, L6.detach(), R6.detach()


def _worst(got, want, scale):
    """max |got - want| / scale; a component whose scale is 0 (no ray reaches it) must be exactly 0."""
    got, want, scale = (np.asarray(a, np.float64).ravel() for a in (got, want, scale))
    assert np.all(np.isfinite(got)), got
    dead = scale == 0
    assert np.all(got[dead] == 0), (got[dead], "gradient where no ray contributes")
    return float((np.abs(got - want)[~dead] / scale[~dead]).max()) if (~dead).any() else 0.0


def _check_case(case, GL, GR, tag, param_list="dp", bar=1e-5, forward_bar=1e-5):
    """The gradients at `bar` x scale, and the forward grids L, R within `forward_bar` of the peak of the restatement
    with float64 fractions -- and, tighter, within 1e-5 of the one with the kernel's own fp32 fractions."""
    theta, gc, L, R = _kernel(case, GL, GR, param_list)
    (wt, wc), (st, sc), _, _ = _restatement(case, GL, GR if param_list == "dp" else None)
    rt = _worst(theta, wt, st) if param_list == "dp" else 0.0
    rc = _worst(gc, wc, sc)
    fwd = {}
    with torch.no_grad():
        for fd in (torch.float64, torch.float32):
            fwd[fd] = splat_f64(*case["rays"], torch.from_numpy(case["cen"]).double(), case["ps"], case["ks"],
                                case["h"], case["f"], case["w"], case["r"], frac_dtype=fd)
    grids = [(L, 0)] + ([(R, 1)] if param_list == "dp" else [])
    err = {fd: [float((g - fwd[fd][k]).abs().max()) for g, k in grids] for fd in fwd}
    peak = {fd: [float(fwd[fd][k].abs().max()) for g, k in grids] for fd in fwd}
    rel = {fd: max(e / max(p, 1e-300) for e, p in zip(err[fd], peak[fd])) for fd in fwd}
    print(f"{tag}: S {case['S']} N {case['N']} ks {case['ks']} r {case['r']:.4f} h {case['h']:.3f} f {case['f']:.3f} "
          f"w {case['w']:.3f} {case['precision']} live {case['n_live']} fragile {case['n_fragile']}: worst "
          f"|got - want| / scale: h,f,w {rt:.2e} centres {rc:.2e}; forward |L, R - restatement| / peak "
          f"{rel[torch.float64]:.2e} (float64 fractions) {rel[torch.float32]:.2e} (fp32 fractions)")
    assert rt <= bar and rc <= bar, (tag, rt, rc)
    for e, p in zip(err[torch.float64], peak[torch.float64]):
        assert e <= forward_bar * p, (tag, e, p)
    for e, p in zip(err[torch.float32], peak[torch.float32]):
        assert e <= 1e-5 * p, (tag, e, p)
    return theta, gc, R


@pytest.mark.parametrize("seed", range(int(os.environ.get("SDIRT_FUZZ_SEEDS", 12))))
def test_random_geometries_and_batch_shapes_against_the_float64_restatement(seed):
    """Fuzz of sdirt_forward_integral_grad: random stacks (h, f, w) and r in thirds (small; big with a u gate that
    closes; big with one that cannot), every launch shape of FUZZ_TABLE, dead and out-of-window rays, random
    upstreams on both grids.  Bar: |got - want| <= 1e-5 x the sum of the per-ray magnitudes, for each of h, f, w and
    every centre component; exactly 0 where no ray contributes.  The forward grids: 1e-5 of the float64
    restatement's peak, but for the one table entry of SPARSE_FORWARD_BAR.

    That entry, 4100 x 3 rays on 150 x 150 pixels, puts at most a ray or two on a pixel, the peak included, so a
    ray's rounding is not averaged out, and it misses 1e-5 by rounding: measured 1.44e-5 of the peak (seed 2), and
    2.5e-7 against the restatement on the kernel's own fp32 fractions.  The operation is the bilinear fraction
    pf - floor(pf): pf is an fp32 number of size <= ks, so what is left of it after the floor carries up to
    ks 2^-23 pixels of rounding (1.8e-5 at ks 150); a tap weight is a product of a row and a column fraction, so a
    single ray's contribution is off by up to 2 ks 2^-23 = 3.6e-5 of itself.  That is the bar there.  Every other
    entry holds 1e-5 (the next largest: 8.4e-6 at 63 x 5 rays and ks 79, 7.0e-6 at ks 79, 6.9e-6 at ks 78)."""
    case = fuzz_case(seed)
    assert fragile_within_cap(case), (case["n_fragile"], case["n_live"])
    GL, GR = _upstreams(case, seed)
    entry = seed % len(FUZZ_TABLE)
    _check_case(case, GL, GR, f"fuzz {seed}",
                forward_bar=2 * case["ks"] * 2.0 ** -23 if entry in SPARSE_FORWARD_BAR else 1e-5)


# ------------------------------------------------------------------ the edges no draw reaches
def test_ray_exactly_on_the_margin_boundary_where_the_reference_autograd_is_not_finite():
    """w = 0.5 = r, x_tan = 0: the margin boundary x2 = w is |x| = r exactly, in fp32 as in float64 (acos' derivative
    is infinite there; the chord is 0).  Finite, and the restatement's."""
    rng = np.random.default_rng(5)
    case = make_case(rng, 16, 2, 5, 0.01, 0.78, 1.44, 0.5, 0.5, "ieee", dead=0.0, x_tan=np.zeros((16, 2)),
                     kill_fragile=False)
    x1, x2 = boundaries(torch.zeros(1, dtype=torch.float64), case["h"], case["f"], case["w"])
    assert float(x2[0]) == 0.5 == case["r"]
    # |x2| = 0.5 is also where the clamp of x2 closes, which is what fragile_rays flags -- but x2 = 0.5 - h * 0 is
    # exact in fp32 as in float64, and both sides pass the gradient on the closed edge: nothing is ambiguous here
    assert case["n_fragile"] == case["n_live"] >= 8
    assert not fragile_rays(*case["rays"], torch.from_numpy(case["cen"]), case["ps"], case["ks"], case["h"], case["f"],
                            case["w"], case["r"], x_band=0.0).any()
    for prec in ("ieee", "lean"):
        case["precision"] = prec
        _check_case(case, *_upstreams(case, 1), f"on |x2| = r, {prec}")


def test_u_clamp_edge_approached_from_both_sides():
    """r = 0.6: |c| = sqrt(r^2 - 1/4) approached to 1e-3 from inside and outside by the middle boundary of x1 and of
    x2, on both signs; the chord is -1 at the edge, the open branch's value."""
    h, f, w, r = (_f32(v) for v in (0.78, 1.44, 0.3, 0.6))
    edge = np.sqrt(r * r - 0.25)
    xs = np.array([s * (edge + e) for s in (1, -1) for e in (1e-3, -1e-3)])
    x_tan = np.concatenate([-xs / h, -xs * (f - h) / (f * h)])              # x2 = -h t ; x1 = -f t h / (f - h)
    rng = np.random.default_rng(6)
    case = make_case(rng, 8, 1, 9, 0.01, h, f, w, r, "lean", dead=0.0, x_tan=np.tile(x_tan, 1).reshape(8, 1))
    case["o"][..., :2] *= 0.5                                              # all inside the window
    case["rays"][0], case["rays"][1] = (torch.from_numpy(np.ascontiguousarray(case["o"][..., k])) for k in (0, 1))
    cen = torch.from_numpy(case["cen"])
    assert not fragile_rays(*case["rays"], cen, case["ps"], 9, h, f, w, r).any()
    case["n_live"] = int(live_in_window(case["rays"][0], case["rays"][1], case["rays"][4], cen, case["ps"], 9).sum())
    assert case["n_live"] == 8
    g = gate_states(torch.from_numpy(x_tan), h, f, w, r)
    assert g["u2"][0][1, :4].tolist() == [False, True, False, True] and g["u2"][1][1, :4].tolist() == [True, False] * 2
    assert g["u1"][0][1, 4:].tolist() == [False, True, False, True] and g["u1"][1][1, 4:].tolist() == [True, False] * 2
    for prec in ("lean", "ieee"):
        case["precision"] = prec
        _check_case(case, *_upstreams(case, 2), f"u edge +-1e-3, {prec}")


def test_fractional_ray_weights_scale_the_position_and_the_taps():
    """ra in [0.25, 1): the weight multiplies the shifted position (monte_carlo.py:38) and the taps, so the centre
    gradients carry it twice and the h, f, w gradients once.  (Traced rays have ra = 0 or 1, where w^2 = w.)"""
    for k, (r, ks, prec) in enumerate([(0.45, 21, "lean"), (0.62, 79, "ieee")]):
        case = make_case(np.random.default_rng(20 + k), 1500, 3, ks, 0.00431, 0.7, 1.5, 0.35, r, prec, weights=True)
        assert fragile_within_cap(case) and len(np.unique(case["ra"])) > 100
        _check_case(case, *_upstreams(case, 20 + k), f"fractional ra, ks {ks}")


def _abi_grad(case, ray, dp, GL, GR, n_slices=None, ks=None, fill=float("nan")):
    """sdirt_forward_integral_grad called directly -> (status, partial [N, slices, 5] float64)."""
    S, N = case["S"], case["N"]
    lib = _lib.lib()
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    ns = int(lib.sdirt_forward_integral_grad_slices(N, S, ncu))
    assert ns >= 1
    rows = ns if n_slices is None else max(ns, n_slices) + 1       # a wrong n_slices gets room to spare
    partial = torch.full((N, rows, 5), fill, dtype=torch.float64, device=DEV)
    dpp = _lib.DpParams(*[float(v) for v in dp]) if dp is not None else None
    cen = _t(case["cen"])
    flags = _lib.PSF_STRICT_IEEE if case["precision"] == "ieee" else 0
    rc = lib.sdirt_forward_integral_grad(
        ray.c_rays(), S, N, float(case["ps"]), int(case["ks"] if ks is None else ks), dptr(cen),
        C.byref(dpp) if dpp is not None else None, flags, dptr(GL), dptr(GR), dptr(partial),
        ns if n_slices is None else n_slices, stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, partial.cpu()


@pytest.mark.parametrize("ks,r", [(21, 0.4), (79, 0.62)])
def test_one_sided_and_absent_upstreams_through_the_c_abi(ks, r):
    """grad_l = NULL is GL = 0 and grad_r = NULL is GR = 0, bit for bit; dp = NULL is the default stack with no
    right grid: its h, f, w partials and centre gradients are those of the left grid alone.  One ks whose grids
    are staged in LDS, one whose grids are read through L2."""
    assert (2 * 4 * ks * ks <= 48 * 1024) == (ks == 21)
    rng = np.random.default_rng(40 + ks)
    case = make_case(rng, 1500, 3, ks, 0.00431, 0.9, 1.7, 0.25, r, "lean")
    ray = _ray(case)
    GL, GR = (g.to(DEV) for g in _upstreams(case, ks))
    Z = torch.zeros_like(GL)
    dp = (case["h"], case["f"], case["w"], case["r"])
    rc, both = _abi_grad(case, ray, dp, GL, GR)
    assert rc == 0 and torch.isfinite(both).all()
    rc_l, no_l = _abi_grad(case, ray, dp, None, GR)
    rc_z, zero_l = _abi_grad(case, ray, dp, Z, GR)
    assert rc_l == 0 == rc_z and torch.equal(no_l, zero_l) and not torch.equal(no_l, both)
    rc_r, no_r = _abi_grad(case, ray, dp, GL, None)
    rc_z, zero_r = _abi_grad(case, ray, dp, GL, Z)
    assert rc_r == 0 == rc_z and torch.equal(no_r, zero_r) and not torch.equal(no_r, both)
    # the two one-sided calls are the two halves of the full one
    assert float((no_l + no_r - both).abs().max()) <= 1e-12 * float(both.abs().max())
    # dp = NULL: the default stack, the right upstream ignored
    default = dict(case, h=0.78, f=1.44, w=0.3, r=0.5)
    rc_n, null = _abi_grad(default, ray, None, GL, GR)
    rc_d, left = _abi_grad(default, ray, (0.78, 1.44, 0.3, 0.5), GL, None)
    assert rc_n == 0 == rc_d and torch.equal(null, left)
    (wt, wc), (st, sc), _, _ = _restatement(default, GL.cpu(), None, frac_dtype=torch.float64)
    tot = null.sum(1).numpy()
    rt, rcn = _worst(tot[:, :3].sum(0), wt, st), _worst(tot[:, 3:], wc, sc)
    print(f"dp = NULL, ks {ks}: worst |got - want| / scale: h,f,w {rt:.2e} centres {rcn:.2e}")
    assert rt <= 1e-5 and rcn <= 1e-5
    # and the full call against the restatement
    (wt, wc), (st, sc), _, _ = _restatement(case, GL.cpu(), GR.cpu(), frac_dtype=torch.float64)
    tot = both.sum(1).numpy()
    assert _worst(tot[:, :3].sum(0), wt, st) <= 1e-5 and _worst(tot[:, 3:], wc, sc) <= 1e-5


def test_default_param_list_sends_the_left_grid_gradient_to_the_centres_and_no_right_grid():
    """param_list=None (the reference's default call): R is all zero, nothing flows back from it, and the centre
    gradients are the restatement's at the default stack."""
    rng = np.random.default_rng(8)
    case = make_case(rng, 1500, 4, 33, 0.00431, *DP, 0.5, "lean")
    GL, GR = _upstreams(case, 8)
    _, _, R = _check_case(case, GL, GR, "param_list=None", param_list=None)
    assert not R.any()


def test_the_slice_count_does_not_change_a_points_gradient():
    """The same 5000 rays as one point alone (several slices) and as every one of thousands of points (one slice
    each): the float64 sums differ in order only, so by at most n eps = 5000 x 1.1e-16 of the sum of the magnitudes
    -- 1e-12 x scale."""
    lib = _lib.lib()
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    S, ks = 5000, 9
    n1 = int(lib.sdirt_forward_integral_grad_slices(1, S, ncu))
    Nb = next((n for n in (3000, 6000, 12000, 375, 100)
               if int(lib.sdirt_forward_integral_grad_slices(n, S, ncu)) != n1), None)
    assert Nb is not None, f"{ncu} CUs: no candidate N changes the slice count of S = {S} from {n1}"
    nb = int(lib.sdirt_forward_integral_grad_slices(Nb, S, ncu))
    print(f"{ncu} CUs: {n1} slices for 1 point, {nb} for {Nb} points")
    assert n1 != nb
    rng = np.random.default_rng(9)
    one = make_case(rng, S, 1, ks, 0.00431, 0.6, 1.5, 0.45, 0.58, "ieee")
    many = dict(one, N=Nb, o=np.tile(one["o"], (1, Nb, 1)), d=np.tile(one["d"], (1, Nb, 1)),
                ra=np.tile(one["ra"], (1, Nb)), cen=np.tile(one["cen"], (Nb, 1)))
    GL, GR = (g.to(DEV) for g in _upstreams(one, 9))
    dp = (one["h"], one["f"], one["w"], one["r"])
    rc1, p1 = _abi_grad(one, _ray(one), dp, GL, GR)
    rcb, pb = _abi_grad(many, _ray(many), dp, GL.expand(Nb, ks, ks).contiguous(), GR.expand(Nb, ks, ks).contiguous())
    assert rc1 == 0 == rcb and p1.shape[1] == n1 and pb.shape[1] == nb
    (wt, wc), (st, sc), _, _ = _restatement(one, GL.cpu(), GR.cpu(), frac_dtype=torch.float64)
    scale = np.concatenate([st, sc.ravel()])
    assert np.all(scale > 0)
    t1, tb = p1.sum(1).numpy()[0], pb.sum(1).numpy()
    assert np.all(tb == tb[0])                                   # every copy of the point: the same bits
    print("slices: |one point - regrouped| / scale", (np.abs(tb[0] - t1) / scale).tolist())
    assert np.all(np.abs(tb - t1) <= 1e-12 * scale)
    assert _worst(t1, np.concatenate([wt, wc.ravel()]), scale) <= 1e-5


@pytest.mark.parametrize("S,N", [(4101, 3), (5003, 1), (2051, 40)])
def test_spp_that_the_slice_count_does_not_divide(S, N):
    """The last slice of every point is shorter than the others (s_end = min(S, ...)): its workgroup must stop at the
    point's last ray, not run on into the next point's.  (The shapes of FUZZ_TABLE all split evenly on 256 CUs.)"""
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    ns = int(_lib.lib().sdirt_forward_integral_grad_slices(N, S, ncu))
    if ns == 1 or S % ns == 0:                   # another CU count: find a neighbour that does not split evenly
        slices = lambda s: int(_lib.lib().sdirt_forward_integral_grad_slices(N, s, ncu))
        S0, S = S, next((s for s in range(S + 1, S + 64) if slices(s) > 1 and s % slices(s) != 0), None)
        assert S is not None, f"{ncu} CUs, N = {N}: no S in ({S0}, {S0 + 64}) is cut into slices of unequal length"
        ns = slices(S)
    assert ns > 1 and S % ns != 0
    case = make_case(np.random.default_rng(S), S, N, 21, 0.00431, 0.8, 1.3, 0.4, 0.55, "lean")
    assert fragile_within_cap(case)
    _check_case(case, *_upstreams(case, S), f"short last slice ({ns} slices)")


def test_bad_arguments_return_the_documented_error_and_write_nothing():
    rng = np.random.default_rng(10)
    case = make_case(rng, 300, 2, 9, 0.00431, *DP, 0.5, "lean")
    ray = _ray(case)
    GL, GR = (g.to(DEV) for g in _upstreams(case, 10))
    lib = _lib.lib()
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    ns = int(lib.sdirt_forward_integral_grad_slices(2, 300, ncu))
    ok = (*DP, 0.5)
    bad = [("n_slices + 1", dict(dp=ok, n_slices=ns + 1), "n_slices"), ("n_slices - 1", dict(dp=ok, n_slices=ns - 1), "n_slices"),
           ("ks 1", dict(dp=ok, n_slices=ns, ks=1), "ks=1 outside"),
           ("ks above the limit", dict(dp=ok, n_slices=ns, ks=_lib.MAX_KS_STAGED + 1), "outside"),
           ("r = 0", dict(dp=(*DP, 0.0), n_slices=ns), "dp->r"), ("r < 0", dict(dp=(*DP, -0.5), n_slices=ns), "dp->r"),
           ("f == h", dict(dp=(0.78, 0.78, 0.3, 0.5), n_slices=ns), "dp->f")]
    for name, kw, text in bad:
        rc, partial = _abi_grad(case, ray, kw.pop("dp"), GL, GR, fill=-7.0, **kw)
        msg = lib.sdirt_last_error().decode()
        assert rc == -1 and text in msg, (name, rc, msg)            # SDIRT_ERR_INVALID_ARGUMENT
        assert bool((partial == -7.0).all()), name
    rc, partial = _abi_grad(case, ray, ok, GL, GR, fill=-7.0, n_slices=ns)      # and the call they all deviate from
    flat, n = partial.reshape(-1), case["N"] * ns * 5
    assert rc == 0 and bool((flat[:n] != -7.0).all()) and bool((flat[n:] == -7.0).all())


# ------------------------------------------------------------------ the Python half by value
PTS_OFF_AXIS = [[0.0, 0.0, -1500.0], [0.3, -0.2, -1200.0], [-0.5, 0.4, -2500.0]]


@pytest.mark.parametrize("r", [0.5, 0.65])
def test_uncentred_psf_lr_gradients_reach_the_points_and_h_by_value(lens, r):
    """psf_lr(points, center=False, normalize=True) with points and h requiring grad: through the pinhole centres
    points[:, :2] * sensor_size / 2 and the max-normalisation, against the restatement on the staged chain's own
    rays.  The centres' VALUES are the chain's fp32 products (one ulp of a centre of some mm is 1e-4 of a pixel);
    their derivative by the points is sensor_size / 2."""
    ks, S = 21, 2048
    torch.manual_seed(11)
    pts0 = torch.tensor(PTS_OFF_AXIS)
    N = pts0.shape[0]
    ray, cen, rays = _staged(lens, pts0, S, center=False)
    pxy = tuple(t.clone() for t in lens.last_pupil_points[:2])
    gen = torch.Generator().manual_seed(12)
    GL, GR = torch.randn((N, ks, ks), generator=gen), torch.randn((N, ks, ks), generator=gen)
    pts = pts0.clone().requires_grad_(True)
    h = torch.tensor(DP[0], requires_grad=True)
    L, R = lens.psf_lr(pts, ks=ks, spp=S, center=False, dp=(h, DP[1], DP[2], r), normalize=True, pupil_xy=pxy)
    ((GL.to(DEV) * L).sum() + (GR.to(DEV) * R).sum()).backward()
    # the restatement, per-ray leaves
    half = torch.tensor([lens.sensor_size[1] / 2, lens.sensor_size[0] / 2], dtype=torch.float64)
    pv = pts0[:, :2].double().unsqueeze(0).expand(S, N, 2).clone().requires_grad_(True)
    hv = torch.full((S, N), float(h), dtype=torch.float64, requires_grad=True)
    cv = cen.cpu().double().unsqueeze(0) + (pv * half - (pv * half).detach())
    f, w = float(np.float32(DP[1])), float(np.float32(DP[2]))
    L6, R6 = splat_f64(*rays, cv, lens.pixel_size, ks, hv, f, w, float(np.float32(r)))
    for g in (L6, R6):                       # the arg-max gradient is well defined: one peak pixel by a clear margin
        top = g.detach().reshape(N, -1).topk(2).values
        print(f"r {r}: (peak - runner-up) / peak per point {((top[:, 0] - top[:, 1]) / top[:, 0]).tolist()}")
        assert bool(((top[:, 0] - top[:, 1]) >= 1e-3 * top[:, 0]).all())
    P6L, P6R = max_normalise(L6), max_normalise(R6)
    assert float((L.detach().cpu() - P6L.detach()).abs().max()) <= 1e-5
    ((GL.double() * P6L).sum() + (GR.double() * P6R).sum()).backward()
    rp = _worst(pts.grad[:, :2].numpy(), pv.grad.sum(0).numpy(), pv.grad.abs().sum(0).numpy())
    rh = _worst([float(h.grad)], [float(hv.grad.sum())], [float(hv.grad.abs().sum())])
    print(f"r {r}: worst |got - want| / scale: points {rp:.2e} h {rh:.2e}")
    assert rp <= 1e-5 and rh <= 1e-5
    assert bool((pts.grad[:, 2] == 0).all()) and bool((pts.grad[:, :2] != 0).all())


@pytest.mark.parametrize("r", [0.5, 0.65])
@pytest.mark.parametrize("direct", ["l", "r"])
def test_psf_diff_direction_picks_the_grid_whose_gradient_it_returns(lens, r, direct):
    pts = torch.tensor(PTS)
    G = torch.randn((len(PTS), 21, 21), generator=torch.Generator().manual_seed(13)).to(DEV)
    h, f, w = _leaves()
    torch.manual_seed(14)
    P = lens.psf_diff(pts, ks=21, spp=2048, param_list=[h, f, w, r, direct])
    (G * P).sum().backward()
    h2, f2, w2 = _leaves()
    torch.manual_seed(14)
    L, R = lens.psf_lr(pts, ks=21, spp=2048, dp=(h2, f2, w2, r))
    assert torch.equal(P.detach(), (L if direct == "l" else R).detach())
    assert not torch.equal(L.detach(), R.detach())
    (G * (L if direct == "l" else R)).sum().backward()
    got, want = [t.grad.item() for t in (h, f, w)], [t.grad.item() for t in (h2, f2, w2)]
    np.testing.assert_allclose(got, want, rtol=1e-6)
    h3, f3, w3 = _leaves()                       # and it is not the other grid's
    torch.manual_seed(14)
    L, R = lens.psf_lr(pts, ks=21, spp=2048, dp=(h3, f3, w3, r))
    (G * (R if direct == "l" else L)).sum().backward()
    assert not np.allclose(got, [t.grad.item() for t in (h3, f3, w3)], rtol=1e-3)
