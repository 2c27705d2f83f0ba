"""The gradient of dual-pixel PSFs in the sensor position (the focus setting) on the GPU: the
six-component splat backward sdirt_forward_integral_grad_focus and the chief-ray pass sdirt_chief_center_slope against
the float64 restatement tests/focus_f64.py (which tests/test_focus_grad_cpu.py holds against the reference's own
autograd), `d_sensor=` on psf_lr / psf_diff / psf_rgb / psf_volume, the chain to an image loss and a fit of the focus
setting.

Bars.  Splat kernel, per point and component: |kernel - float64| <= 1e-5 sum|per-ray terms| (7d's bar for this kernel
family).  Centre slope: (2048 + 8) 2^-53 sum|terms| / (sum ra + 1e-9): the order-dependent rounding of 2048 float64
additions, the terms themselves being the same float64 operations on the same fp32 rays.  d_sensor.grad: the splat
kernel's bar on the per-ray terms of the whole graph (each ray's own share and its share of the centre's motion)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import focus_f64 as F
from conftest import DATA, ROOT, load_state, make_lens
from splat_f64 import max_normalise

from sdirt_amd import _lib
from sdirt_amd.basics import DEFAULT_WAVE, GEO_SPP, WAVE_RGB, dptr, stream_ptr

sys.path.insert(0, os.path.join(ROOT, "tools"))
import focus_adam_f64 as adam_problem  # noqa: E402  (the fit's problem definition; importing it needs no reference)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = tuple(float(np.float32(v)) for v in (0.78, 1.44, 0.3))
KS, SPP = 21, 512


def _r32(r):
    return float(np.float32(r))


@pytest.fixture(scope="module")
def lens():
    return make_lens("rf50mm", DEV, load_state("rf50mm"))


def _staged(lens, pts, spp, center, pupil_xy=None, center_pupil_xy=None, wvln=DEFAULT_WAVE):
    """The staged chain's own sensor-plane rays (the bundle, and ox, oy, dx, dy, dz, ra as CPU [S, N]) and centres."""
    N = pts.shape[0]
    with torch.no_grad():
        po = lens._points_to_object(pts)
        cen = torch.empty((N, 2), dtype=torch.float32, device=DEV)
        ray, spp = lens._staged_rays(pts, po, N, wvln, spp, center, pupil_xy, center_pupil_xy, cen)
    soa = ray.soa[:, :spp * N].view(-1, N, spp).transpose(1, 2)          # point-major -> [7, S, N]
    return ray, cen, [soa[k].cpu() for k in (0, 1, 3, 4, 5, 6)]


def _chief_rays(lens, pts, center_pupil_xy):
    """The green chief rays of `pts` at the sensor through the staged API: sampled on the shrunk pupil's points (the
    pupil plane is the same), traced and propagated.  -> ox, oy, dx, dy, dz, ra, CPU [Sc, N]."""
    return _staged(lens, pts, center_pupil_xy[0].shape[0], False, center_pupil_xy)[2]


def _slope_f64(chief):
    """(dc/ds [N, 2], sum|terms| / den [N, 2]) in float64 torch from the chief rays."""
    terms = F.chief_slope_terms(*chief[2:])
    den = chief[5].double().sum(0).unsqueeze(-1) + 1e-9
    return -terms.sum(0) / den, terms.abs().sum(0) / den


# ------------------------------------------------------------------ the six-component entry
def _entry(name, comps, ray, S, N, ps, ks, cen, dp, prec, gl, gr):
    lib = _lib.lib()
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    ns = int(lib.sdirt_forward_integral_grad_slices(N, S, ncu))
    partial = torch.full((N, ns, comps), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(getattr(lib, name)(ray.c_rays(), S, N, float(ps), int(ks), dptr(cen), C.byref(dp),
                                  _lib.PSF_STRICT_IEEE if prec == "ieee" else 0, dptr(gl), dptr(gr), dptr(partial), ns,
                                  stream_ptr(DEV)))
    return partial, ns


@pytest.mark.parametrize("N,S,ks,prec,r,sides", [
    (3, 300, 21, "lean", 0.5, "lr"), (3, 300, 150, "ieee", 0.65, "lr"), (3, 300, 21, "ieee", 0.65, "l"),
    (2, 70000, 21, "ieee", 0.5, "l"), (2, 70000, 150, "lean", 0.65, "r"), (2, 70000, 21, "lean", 0.65, "lr"),
    (2, 70000, 150, "ieee", 0.5, "lr")])
def test_six_component_entry_against_the_restatement_and_the_five_component_entry(lens, N, S, ks, prec, r, sides):
    """On the staged chain's own rays.  300 spp: one slice, a ragged last wave; 70 000 spp: several slices.  ks 21:
    the grids staged in LDS; ks 150: read through L2.  Components 0-4 are sdirt_forward_integral_grad's bits."""
    torch.manual_seed(11)
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.4, -0.3, -1200.0], [-0.7, 0.5, -2500.0]])[:N]
    ray, cen, rays = _staged(lens, pts, S, True)
    gen = torch.Generator().manual_seed(ks + S)
    GL, GR = torch.randn((N, ks, ks), generator=gen), torch.randn((N, ks, ks), generator=gen)
    gl = GL.to(DEV) if "l" in sides else None
    gr = GR.to(DEV) if "r" in sides else None
    r = _r32(r)
    dp = _lib.DpParams(*DP, r)
    p6, ns = _entry("sdirt_forward_integral_grad_focus", 6, ray, S, N, lens.pixel_size, ks, cen, dp, prec, gl, gr)
    p5, _ = _entry("sdirt_forward_integral_grad", 5, ray, S, N, lens.pixel_size, ks, cen, dp, prec, gl, gr)
    assert (ns > 1) == (S == 70000) and (2 * ks * ks * 4 <= 48 * 1024) == (ks == 21)
    assert not torch.isnan(p6).any()
    assert torch.equal(p6[..., :5].contiguous().view(torch.int64), p5.view(torch.int64))
    got = p6.sum(1).cpu().numpy()                                                   # [N, 6]
    # the restatement with per-ray leaves: the sum of their gradients is the gradient, the sum of |.| the scale
    s0 = float(lens.d_sensor)
    hv, fv, wv = (torch.full((S, N), v, dtype=torch.float64, requires_grad=True) for v in DP)
    sv = torch.full((S, N), s0, dtype=torch.float64, requires_grad=True)
    cv = cen.cpu().double().unsqueeze(0).expand(S, N, 2).clone().requires_grad_(True)
    L6, R6 = F.raw_psf(rays, sv, s0, cv, lens.pixel_size, ks, hv, fv, wv, r)
    loss = sum((G.double() * P).sum() for G, P, k in ((GL, L6, "l"), (GR, R6, "r")) if k in sides)
    loss.backward()
    per_ray = [hv.grad, fv.grad, wv.grad, cv.grad[..., 0], cv.grad[..., 1], sv.grad]
    want = torch.stack([g.sum(0) for g in per_ray], -1).numpy()
    scale = torch.stack([g.abs().sum(0) for g in per_ray], -1).numpy()
    assert np.all(scale > 0)
    worst = np.abs(got - want) / scale
    print(f"N {N} S {S} ks {ks} {prec} r {r:.2f} sides {sides}: slices {ns}, worst |kernel - float64| / sum|terms| per "
          f"component {worst.max(0)}")
    assert np.all(np.abs(got - want) <= 1e-5 * scale), (got, want, worst)


# ------------------------------------------------------------------ the chief-ray pass with the centre's slope
def test_slope_entry_writes_the_same_centre_and_the_float64_sum_of_the_chief_rays(lens):
    """On axis and a field corner at 0.3 m, one point between and one past the corner (where chief rays may die: a dead
    ray contributes nothing, whatever direction the trace left it with)."""
    torch.manual_seed(5)
    pts = torch.tensor([[0.0, 0.0, -300.0], [0.98, 0.98, -300.0], [-0.5, 0.3, -1500.0], [1.2, 1.2, -300.0]])
    N = pts.shape[0]
    with torch.no_grad():
        po = lens._points_to_object(pts)
        pz, pr = lens.entrance_pupil(shrink_pupil=True)
        xc, yc = lens._pupil_samples(GEO_SPP, pr)
        cen0 = torch.empty((N, 2), dtype=torch.float32, device=DEV)
        cen1 = torch.full_like(cen0, float("nan"))
        slope = torch.full((N, 2), float("nan"), dtype=torch.float64, device=DEV)
        lens._chief_center(po, xc, yc, pz, cen0)
        lens._chief_center(po, xc, yc, pz, cen1, slope)
    assert torch.equal(cen0.view(torch.int32), cen1.view(torch.int32))
    chief = _chief_rays(lens, pts, (xc, yc))
    assert chief[0].shape == (GEO_SPP, N) and float(chief[5][:, 0].min()) == 1.0
    print(f"live chief rays per point: {chief[5].sum(0).tolist()}")
    want, scale = _slope_f64(chief)
    got = slope.cpu()
    bar = (2048 + 8) * 2.0 ** -53 * scale
    print(f"dc/ds {got.tolist()}; |kernel - float64 sum| / bar {((got - want).abs() / bar).tolist()}")
    assert bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= bar).all())
    assert float(got[1].abs().min()) > 1e-3                   # the corner's centre moves with the sensor


# ------------------------------------------------------------------ d_sensor= on the Python calls
def _pupils(lens, spp=SPP, seed=23):
    g = torch.Generator().manual_seed(seed)
    u = [torch.rand(n, generator=g) for n in (spp, spp, GEO_SPP, GEO_SPP)]
    pr = lens.entrance_pupil()[1]
    pxy = tuple(t.to(DEV) for t in adam_problem.pupil_points(u[0], u[1], pr))
    cxy = tuple(t.to(DEV) for t in adam_problem.pupil_points(u[2], u[3], pr * 0.25))
    return pxy, cxy


def _points(lens):
    pts = torch.tensor(adam_problem.POINTS)
    pts[:, 2] += float(lens.d_sensor)
    return pts


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_a_plain_sensor_position_is_set_state_followed_by_the_call_and_the_lens_is_put_back(lens):
    pts, (pxy, cxy) = _points(lens), _pupils(lens)
    old = lens.d_sensor
    v = float(np.float32(old + 0.03))
    rgb_p = torch.stack([torch.stack([pxy[0]] * 3), torch.stack([pxy[1]] * 3)])
    rgb_c = torch.stack([torch.stack([cxy[0]] * 3), torch.stack([cxy[1]] * 3)])
    calls = {
        "fused": lambda **kw: lens.psf_lr(pts, ks=KS, pupil_xy=pxy, center_pupil_xy=cxy, **kw),
        "uncentred": lambda **kw: lens.psf_lr(pts, ks=KS, center=False, pupil_xy=pxy, **kw),
        "psf_diff": lambda **kw: (lens.psf_diff(pts, ks=KS, spp=SPP, param_list=[*DP, 0.5, "r"], **kw),),
        "psf_rgb": lambda **kw: (lens.psf_rgb(pts, ks=KS, param_list=[*DP, 0.5, "l"], pupil_xy=rgb_p, center_pupil_xy=rgb_c, **kw),),
        "psf_rgb uncentred": lambda **kw: (lens.psf_rgb(pts, ks=KS, center=False, param_list=[*DP, 0.5, "l"], pupil_xy=rgb_p, **kw),),
    }
    with torch.no_grad():
        for name, call in calls.items():
            for form in (v, torch.tensor(v), torch.tensor(v, requires_grad=True)):
                torch.manual_seed(1)
                got = call(d_sensor=form)
                assert lens.d_sensor == old, name
                try:
                    lens.set_state(d_sensor=v)
                    torch.manual_seed(1)
                    want = call()
                finally:
                    lens.set_state(d_sensor=old)
                torch.manual_seed(1)
                plain = call()
                for a, b, c in zip(got, want, plain):
                    assert torch.equal(_bits(a), _bits(b)), name
                    assert not torch.equal(_bits(a), _bits(c)), name      # and the sensor position matters
        with pytest.raises(Exception):
            lens.psf_lr(pts, ks=1, pupil_xy=pxy, center_pupil_xy=cxy, d_sensor=v)
    assert lens.d_sensor == old
    # a tensor that requires a gradient, in grad mode, of a call that then raises
    with pytest.raises(ValueError):
        lens.psf_lr(pts, ks=KS, pupil_xy=pxy, center_pupil_xy=cxy, d_sensor=torch.tensor(v, requires_grad=True), defer=True)
    assert lens.d_sensor == old


def test_psfs_under_grad_are_the_existing_grad_paths_on_a_lens_set_to_that_position(lens):
    pts, (pxy, cxy) = _points(lens), _pupils(lens)
    old = lens.d_sensor
    t = torch.tensor(old + 0.03, requires_grad=True)
    for center in (True, False):
        kw = dict(ks=KS, center=center, pupil_xy=pxy, center_pupil_xy=cxy if center else None)
        Lg, Rg = lens.psf_lr(pts, dp=(*DP, 0.5), d_sensor=t, **kw)
        assert Lg.grad_fn is not None and lens.d_sensor == old
        try:
            lens.set_state(d_sensor=float(t.detach()))
            L0, R0 = lens.psf_lr(pts, dp=(torch.tensor(DP[0], requires_grad=True), *DP[1:], 0.5), **kw)
        finally:
            lens.set_state(d_sensor=old)
        assert torch.equal(_bits(Lg), _bits(L0)) and torch.equal(_bits(Rg), _bits(R0))


def test_h_and_points_gradients_do_not_change_when_the_sensor_gets_one_too(lens):
    (pxy, _), G = _pupils(lens), torch.randn((4, KS, KS), generator=torch.Generator().manual_seed(2)).to(DEV)
    v = float(np.float32(lens.d_sensor + 0.03))
    out = []
    for sensor in (torch.tensor(v, requires_grad=True), v):
        pts = _points(lens).requires_grad_(True)
        h = torch.tensor(DP[0], requires_grad=True)
        L, R = lens.psf_lr(pts, ks=KS, center=False, dp=(h, *DP[1:], 0.5), pupil_xy=pxy, d_sensor=sensor)
        ((G * L).sum() - (G * R).sum()).backward()
        out.append((h.grad.clone(), pts.grad.clone()))
        assert float(h.grad) != 0.0 and float(pts.grad[:, :2].abs().max()) > 0
    assert out[0][0].item() == out[1][0].item() and torch.equal(_bits(out[0][1]), _bits(out[1][1]))


def _sensor_grad_against_restatement(lens, pts, center, r, v, pxy, cxy, surface_params=None, wvln=DEFAULT_WAVE):
    """(t.grad, the restatement's value, its scale, the other leaves) of sum(G_l L) + sum(G_r R) over psf_lr(d_sensor=t)."""
    N = pts.shape[0]
    gen = torch.Generator().manual_seed(31)
    GL, GR = torch.randn((N, KS, KS), generator=gen), torch.randn((N, KS, KS), generator=gen)
    t = torch.tensor(v, requires_grad=True)
    assert float(t) == v
    L, R = lens.psf_lr(pts, ks=KS, wvln=wvln, center=center, dp=(*DP, r), pupil_xy=pxy,
                       center_pupil_xy=cxy if center else None, d_sensor=t, surface_params=surface_params)
    ((GL.to(DEV) * L).sum() + (GR.to(DEV) * R).sum()).backward()
    # the restatement on the staged chain's own rays with the sensor at v; every primary ray has its own leaf, which moves
    # its own point and its copy of the centre: its gradient is the ray's term of the whole graph
    with lens._sensor_borrowed(v):
        _, cen, rays = _staged(lens, pts, pxy[0].shape[0], center, pxy, cxy if center else None, wvln)
        chief = _chief_rays(lens, pts, cxy) if center else None
    S = rays[0].shape[0]
    sv = torch.full((S, N), v, dtype=torch.float64, requires_grad=True)
    cv = cen.cpu().double().unsqueeze(0).expand(S, N, 2)
    if center:
        cv = cv + _slope_f64(chief)[0].unsqueeze(0) * (sv - v).unsqueeze(-1)
    L6, R6 = F.raw_psf(rays, sv, v, cv, lens.pixel_size, KS, *DP, _r32(r))
    ((GL.double() * max_normalise(L6)).sum() + (GR.double() * max_normalise(R6)).sum()).backward()
    assert float((L.detach().cpu() - max_normalise(L6).detach()).abs().max()) < 1e-5
    return float(t.grad), float(sv.grad.sum()), float(sv.grad.abs().sum())


@pytest.mark.parametrize("center,r", [(True, 0.5), (False, 0.5), (True, 0.65)])
def test_sensor_gradient_against_the_restatements_autograd(lens, center, r):
    pts, (pxy, cxy) = _points(lens), _pupils(lens)
    v = float(np.float32(lens.d_sensor + 0.03))
    got, want, scale = _sensor_grad_against_restatement(lens, pts, center, r, v, pxy, cxy)
    print(f"center {center} r {r}: d loss / d d_sensor = {got:+.6e}, float64 {want:+.6e}, |difference| / sum|terms| = "
          f"{abs(got - want) / scale:.2e}")
    assert want != 0.0 and abs(got - want) <= 1e-5 * scale
    assert lens.d_sensor == load_state("rf50mm")["d_sensor"]


def test_sensor_gradient_together_with_surface_params_on_rf35mm():
    """theta.grad is what it is without a gradient in the sensor position (for the surfaces d_sensor and the centres stay
    constants, 7f), and d_sensor.grad meets the restatement on the borrowed lens's rays."""
    lens = make_lens("rf35mm", DEV, load_state("rf35mm"))
    pts = torch.tensor([[0.0, 0.0, -1500.0], [0.35, -0.2, -1200.0], [-0.6, 0.45, -2500.0], [0.5, 0.6, -900.0]])
    (pxy, cxy) = _pupils(lens)
    v = float(np.float32(lens.d_sensor + 0.02))
    theta = lens.surface_parameters().requires_grad_(True)
    got, want, scale = _sensor_grad_against_restatement(lens, pts, True, 0.5, v, pxy, cxy, surface_params=theta)
    print(f"rf35mm with surface_params: d loss / d d_sensor = {got:+.6e}, float64 {want:+.6e}, |difference| / sum|terms| "
          f"= {abs(got - want) / scale:.2e}")
    assert want != 0.0 and abs(got - want) <= 1e-5 * scale
    theta2 = lens.surface_parameters().requires_grad_(True)
    gen = torch.Generator().manual_seed(31)
    GL, GR = torch.randn((4, KS, KS), generator=gen).to(DEV), torch.randn((4, KS, KS), generator=gen).to(DEV)
    L, R = lens.psf_lr(pts, ks=KS, dp=(*DP, 0.5), pupil_xy=pxy, center_pupil_xy=cxy, d_sensor=v, surface_params=theta2)
    ((GL * L).sum() + (GR * R).sum()).backward()
    assert float(theta.grad.abs().max()) > 0 and torch.equal(_bits(theta.grad), _bits(theta2.grad))
    assert lens.d_sensor == load_state("rf35mm")["d_sensor"]


def test_two_backward_passes_give_the_same_bits(lens):
    pts, (pxy, cxy) = _points(lens), _pupils(lens)
    G = torch.randn((4, KS, KS), generator=torch.Generator().manual_seed(2)).to(DEV)
    out = []
    for _ in range(2):
        t = torch.tensor(lens.d_sensor + 0.03, requires_grad=True)
        L, R = lens.psf_lr(pts, ks=KS, dp=(*DP, 0.65), pupil_xy=pxy, center_pupil_xy=cxy, d_sensor=t)
        ((G * L).sum() + (G * R).sum()).backward()
        out.append(t.grad.item())
    assert out[0] == out[1] and out[0] != 0.0


def test_psf_rgb_gradient_is_the_sum_of_its_three_calls(lens):
    pts, (pxy, cxy) = _points(lens), _pupils(lens)
    P = torch.stack([torch.stack([pxy[0]] * 3), torch.stack([pxy[1]] * 3)])          # [2, 3, spp]
    Pc = torch.stack([torch.stack([cxy[0]] * 3), torch.stack([cxy[1]] * 3)])
    G = torch.randn((4, 3, KS, KS), generator=torch.Generator().manual_seed(3)).to(DEV)
    v = lens.d_sensor + 0.03
    t = torch.tensor(v, requires_grad=True)
    rgb = lens.psf_rgb(pts, ks=KS, param_list=[*DP, 0.5, "r"], pupil_xy=P, center_pupil_xy=Pc, d_sensor=t)
    (G * rgb).sum().backward()
    want = 0.0
    for k, wv in enumerate(WAVE_RGB):
        t2 = torch.tensor(v, requires_grad=True)
        _, R = lens.psf_lr(pts, ks=KS, wvln=wv, dp=(*DP, 0.5), pupil_xy=(P[0][k], P[1][k]),
                           center_pupil_xy=(Pc[0][k], Pc[1][k]), d_sensor=t2)
        (G[:, k] * R).sum().backward()
        want += t2.grad.item()
    np.testing.assert_allclose(t.grad.item(), want, rtol=1e-6)
    with torch.no_grad():                                   # and the values are the fused call's
        ref = lens.psf_rgb(pts, ks=KS, param_list=[*DP, 0.5, "r"], pupil_xy=P, center_pupil_xy=Pc, d_sensor=v)
    assert float((rgb.detach() - ref).abs().max()) <= 1e-6


@pytest.mark.parametrize("kw", ["defer", "out", "center_out"])
def test_grad_calls_in_the_sensor_position_refuse_defer_out_and_center_out(lens, kw):
    pts, (pxy, cxy) = _points(lens), _pupils(lens)
    extra = {"defer": dict(defer=True),
             "out": dict(out=(torch.empty((4, KS, KS), device=DEV), torch.empty((4, KS, KS), device=DEV))),
             "center_out": dict(center_out=torch.empty((4, 2), device=DEV))}[kw]
    with pytest.raises(ValueError):
        lens.psf_lr(pts, ks=KS, pupil_xy=pxy, center_pupil_xy=cxy, d_sensor=torch.tensor(lens.d_sensor, requires_grad=True),
                    **extra)
    assert lens.d_sensor == load_state("rf50mm")["d_sensor"]


# ------------------------------------------------------------------ the chain to an image loss
def test_gradient_reaches_the_sensor_position_through_psf_volume_and_render_volume():
    """psf_volume(grid (3, 4), z 3, ks 11, spp 1024, d_sensor=t) -> PSFNet.render_volume on a 12 x 16 image -> L2 loss.
    t.grad is within 2 max(s, 1e-4) relative of the composed path's (torch interpolation + local_dp_psf_render on
    materialised kernels), s the composed path's own spread: its fp32 render stage against the same graph with that
    stage's gradient from the float64 restatement (7g's rule for h.grad)."""
    from render_volume_f64 import interpolate_kernels, render_volume_f64
    from sdirt_amd.psfnet import PSFNet
    from sdirt_amd.render_psf import local_dp_psf_render, volume_segment_tables
    ks, H, W, C_ = 11, 12, 16, 3
    net = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=ks, device=DEV)
    net.refocus(-1000 + net.d_sensor)
    d0 = float(np.float32(net.d_sensor))
    torch.manual_seed(3)
    with torch.no_grad():
        net.psf_lr(torch.tensor([[0.0, 0.0, -1500.0]]), ks=ks, spp=1024)
    pupil = tuple(t.clone() for t in net.last_pupil_points)
    volume = lambda s: net.psf_volume(grid=(3, 4), z=3, ks=ks, spp=1024, d_sensor=s, pupil_xy=pupil[:2],
                                      center_pupil_xy=pupil[2:])
    gen = torch.Generator().manual_seed(4)
    img = (0.1 + 0.8 * torch.rand((1, C_, H, W), generator=gen)).to(DEV)
    ramp = torch.linspace(0, 1, W).reshape(1, 1, 1, W) * 0.7 + torch.linspace(0, 1, H).reshape(1, 1, H, 1) * 0.3
    depth = (-1000.0 - 14000.0 * ramp).to(DEV) - net.d_sensor
    with torch.no_grad():
        target = net.render_volume(img, depth, volume(d0 + 0.05))
    loss_of = lambda out: ((out - target) ** 2).sum()

    t = torch.tensor(d0, requires_grad=True)
    vol = volume(t)
    assert vol.psf.shape == (3, 3, 4, 2, ks, ks) and vol.psf.grad_fn is not None
    loss_of(net.render_volume(img, depth, vol)).backward()
    assert t.grad is not None
    g_fused = float(t.grad)

    t2 = torch.tensor(d0, requires_grad=True)
    vol2 = volume(t2)
    z = net.depth2z(depth + net.d_sensor).squeeze(1)
    tables = volume_segment_tables(vol2.x_nodes, vol2.y_nodes, vol2.z_nodes, z, H, W)
    lin = net.degamma(img)
    out2 = torch.clip(net.gamma(local_dp_psf_render(lin, interpolate_kernels(vol2.psf, tables), ks)), 0.0, 1.0)
    # the same graph with the render stage's gradient from the float64 restatement
    v64 = vol2.psf.detach().cpu().double().requires_grad_(True)
    l64, r64 = render_volume_f64(lin.cpu(), v64, tuple(x.cpu() for x in tables), ks)
    ((torch.clip(net.gamma(torch.cat([l64, r64], 1)), 0.0, 1.0) - target.cpu().double()) ** 2).sum().backward()
    (g_f64,) = torch.autograd.grad(vol2.psf, t2, grad_outputs=v64.grad.float().to(DEV), retain_graph=True)
    loss_of(out2).backward()
    g_composed, g_f64 = float(t2.grad), float(g_f64)
    s = abs(g_composed - g_f64) / abs(g_f64)
    rel = abs(g_fused - g_composed) / abs(g_composed)
    print(f"d loss / d d_sensor: fused {g_fused:.9e}, composed {g_composed:.9e}, composed with the float64 render gradient "
          f"{g_f64:.9e}; spread s = {s:.3e}, |fused - composed| / |composed| = {rel:.3e}, allowed {2 * max(s, 1e-4):.3e}")
    assert np.isfinite(g_fused) and g_fused != 0.0
    assert rel <= 2 * max(s, 1e-4)


# ------------------------------------------------------------------ fitting the focus setting
def test_adam_recovers_the_sensor_position(lens):
    """A target pair rendered at d_sensor + 0.05 mm; Adam on the sensor position alone from d_sensor, fixed pupil
    samples, 12 steps of 8e-3 mm falling linearly to 0 (tools/focus_adam_f64.py: the same problem in float64 on the CPU
    with the restatement, where the loss falls monotonically to 0.0040 of its first value and |t - truth| to 0.058 of
    the offset).  Asserted with 7f's margin of 1.4: 0.0056 and 0.081."""
    A = adam_problem
    d0 = float(lens.d_sensor)
    pts, pxy, cxy = A.problem(d0, lens.entrance_pupil()[1])
    pxy, cxy = tuple(x.to(DEV) for x in pxy), tuple(x.to(DEV) for x in cxy)
    kw = dict(ks=A.KS, dp=A.DP, pupil_xy=pxy, center_pupil_xy=cxy)
    with torch.no_grad():
        tL, tR = lens.psf_lr(pts, d_sensor=d0 + A.OFFSET, **kw)

    def loss_at(t):
        L, R = lens.psf_lr(pts, d_sensor=t, **kw)
        return ((L - tL) ** 2).sum() + ((R - tR) ** 2).sum()
    losses, dist = A.adam(loss_at, d0, d0 + A.OFFSET)
    print("losses", " ".join(f"{v:.4e}" for v in losses))
    print(f"loss ratio last / first = {losses[-1] / losses[0]:.4f}   |t - truth| / offset = {dist / A.OFFSET:.4f}")
    assert losses[-1] / losses[0] <= 0.0056 and dist / A.OFFSET <= 0.081
    assert lens.d_sensor == d0
