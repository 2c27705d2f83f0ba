"""Gradients of dual-pixel PSFs in the OBJECT POINTS on the GPU: psf_lr / psf_diff / psf_rgb with point_grad=True
(sdirt_trace2sensor_grad_points, trace_grad.PointGradFunction / ChiefCentreFunction).

A. The entry against the float64 restatement (tests/point_f64.py) on the kernel's own fp32 checkpoints, trip tables and
   per-ray upstream gradients: per point and component |kernel - float64| <= TOL * sum |per-ray terms|.
B. The whole call against the restatement's autograd; the chief-ray Jacobian against differences of sdirt_chief_center.
C. Properties: bit-equal forwards and centres, determinism, exact zeros, the sum rules, untouched other gradients.
D. Depth by descent.

TOL = 2 * max(spread, 1e-4) is the rule of DESIGN.md 7d/7f; the spread of the reference's own fp32-against-float64
autograd in the same normalised form is measured by tools/gen_point_grad.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import point_f64 as P
import trace_f64 as T
from conftest import load_state, make_lens
from splat_f64 import max_normalise
from test_gpu_trace_grad import _points

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from sdirt_amd import _lib
from sdirt_amd import trace_grad as TGm
from sdirt_amd.basics import DEFAULT_WAVE, WAVE_RGB, Ray, dptr, stream_ptr
from sdirt_amd.monte_carlo import _flags, splat_autograd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
SPREAD = 4.52e-4         # tools/gen_point_grad.py: the reference's fp32 against its float64 autograd, worst case and component
TOL = 2 * max(SPREAD, 1e-4)
REPEATABLE_SPP = 1000    # below 1024 samples one workgroup owns a point's spp axis: the forward repeats bit for bit (7f)
CORNERS = {"rf50mm": 0.98, "rf35mm": 1.08}


def _lens(name):
    return make_lens(name, DEV, load_state(name))


def _corner_points(name):
    f = CORNERS[name]
    return torch.tensor([[f, f, -300.0], [-f, f, -20000.0], [f, -f, -500.0], [-f, -f, -300.0],
                         [0.0, 0.98, -300.0], [0.98, 0.0, -20000.0], [0.0, 0.0, -1500.0], [0.7, 0.7, -300.0]])


def _disc(radius, n, seed):
    """n points of the disc of `radius`, as sample_from_points maps its uniforms: (x, y) fp32 on the device."""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(n, generator=g) * 2 * np.pi
    rad = torch.sqrt(torch.rand(n, generator=g) * float(radius) ** 2)
    return (rad * torch.cos(ang)).to(DEV), (rad * torch.sin(ang)).to(DEV)


def _samples(lens, x, y, shrink=False):
    return TGm.PointSamples(x, y, lens.entrance_pupil(shrink_pupil=shrink)[0], np.tan(lens.hfov), lens.r_last,
                            lens.sensor_size[1], lens.sensor_size[0])


def _record(lens, pts, x2, y2, wvln=DEFAULT_WAVE, shrink=False):
    """The recorded bundle of the points: (object points [N, 3] fp32, TraceRecord)."""
    po = lens._points_to_object_now(pts)
    S, N = x2.shape[0], pts.shape[0]
    ray = Ray.empty((S, N), wvln, lens.device)
    _lib.check(_lib.lib().sdirt_sample_rays(dptr(po), N, dptr(x2), dptr(y2), S, float(lens.entrance_pupil(shrink_pupil=shrink)[0]),
                                            ray.c_rays(), stream_ptr(lens.device)))
    return po, lens._trace2sensor_recorded(ray)


def _slices(N, S):
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    return int(_lib.lib().sdirt_forward_integral_grad_slices(N, S, ncu))


def _ray_grad(rec, cen, ps, ks, GL, GR, dp=DP):
    """sdirt_forward_integral_grad_rays on the recorded bundle: [4, M] float32."""
    S, N = rec.ray.shape
    out = torch.full((4, S * N), float("nan"), dtype=torch.float32, device=DEV)
    dpp = _lib.DpParams(*[float(v) for v in dp])
    _lib.check(_lib.lib().sdirt_forward_integral_grad_rays(rec.ray.c_rays(), S, N, float(ps), ks, dptr(cen), C.byref(dpp),
                                                           _flags(rec.precision), dptr(GL), dptr(GR), None, _slices(N, S),
                                                           dptr(out), stream_ptr(torch.device(DEV))))
    return out


def _restated_p_bar(lens, rec, ray_grad, x2, y2, pupil_z, wvln=DEFAULT_WAVE, chunk=1 << 16):
    """(p_bar, sum of |per-ray terms|) [N, 3] float64 of sum_rays ray_grad . (o.x, o.y, d.x, d.z) at the sensor as a
    function of the object points, by the restatement on the kernel's checkpoints: every ray has its own copy of its
    point as a leaf.  On the GPU, in chunks of rays."""
    S, N = rec.ray.shape
    K, M = rec.n_surfaces, S * N
    ws = rec.workspace.view(K + 1, 6, M)
    ra = rec.ray.soa[6, :M]
    idx = torch.nonzero((ra != 0) & (ray_grad != 0).any(0)).reshape(-1)
    theta, table = lens.surface_parameters().double().to(DEV), T.lens_table(lens, wvln)
    tot = torch.zeros((N, 3), dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(tot)
    for a in range(0, idx.numel(), chunk):
        ii = idx[a:a + chunk]
        ck = ws[:, :, ii]
        p = ck[0, :3].t().double().clone().requires_grad_()                      # checkpoint 0's o: the point itself
        q = torch.stack((x2[ii % S].double(), y2[ii % S].double(), torch.full_like(p[:, 0], float(np.float32(pupil_z)))), -1)
        v = q - p
        so, sd = T.trace_f64(p, v / v.norm(dim=-1, keepdim=True), theta, table, rec.trips, rec.d_sensor, checkpoints=ck)
        g = ray_grad[:, ii].double()
        (g[0] * so[:, 0] + g[1] * so[:, 1] + g[2] * sd[:, 0] + g[3] * sd[:, 2]).sum().backward()
        tot.index_add_(0, ii // S, p.grad)
        mag.index_add_(0, ii // S, p.grad.abs())
    return tot, mag, int(idx.numel())


ENTRY_CASES = [("rf50mm", "lean", 3, 1), ("rf50mm", "ieee", 3, 63), ("rf35mm", "lean", 3, 257), ("rf50mm", "lean", 1, 20000),
               ("rf35mm", "ieee", 2, 20000), ("rf50mm", "lean", "corners", 4096), ("rf35mm", "ieee", "corners", 4096),
               ("rf50mm", "ieee", "corners", 4096), ("rf35mm", "lean", "corners", 4096)]


@pytest.mark.parametrize("name, precision, N, S", ENTRY_CASES)
def test_entry_matches_float64_restatement(name, precision, N, S):
    lens = _lens(name)
    lens.precision = precision
    corners = N == "corners"
    pts = _corner_points(name) if corners else _points(N)
    N = pts.shape[0]
    pupil_z, pupil_r = lens.entrance_pupil()
    x2, y2 = _disc(pupil_r * (1.0 if corners else 0.8), S, seed=31)
    po, rec = _record(lens, pts, x2, y2)
    M = S * N
    ra = rec.ray.soa[6, :M]
    dead = float((ra == 0).float().mean())
    assert dead <= 0.15, dead
    if corners:
        assert dead > 0.0
    rg = torch.randn((4, M), generator=torch.Generator().manual_seed(6)).to(DEV) * (ra != 0)
    if N > 1:
        rg.view(4, N, S)[:, N - 1] = 0                                                   # the last point: no live ray
    if S >= 20000:
        assert _slices(N, S) > 1
    smp = _samples(lens, x2, y2)
    got = TGm.points_bar(rec, rg, smp)
    again = TGm.points_bar(rec, rg, smp)
    assert torch.equal(got, again)
    want, mag, n_live = _restated_p_bar(lens, rec, rg, x2, y2, pupil_z)
    err = (got - want).abs() / mag.clamp_min(1e-300)
    live_pts = mag[:, 0] > 0
    print(f"{name} {precision} N {N} S {S}: dead {dead:.3f} slices {_slices(N, S)} trips {rec.trips} "
          f"max |kernel - f64| / sum|terms| = {float(err[live_pts].max()):.3e}")
    assert bool(torch.isfinite(got).all()) and n_live > 0
    if N > 1:
        assert not bool(live_pts[N - 1]) and bool((got[N - 1] == 0).all())            # exact zeros
    assert float(err[live_pts].max()) <= TOL
    # the checkpoint the kernel takes the point from is the object point
    assert torch.equal(rec.workspace.view(rec.n_surfaces + 1, 6, M)[0, :3, ::S].t().contiguous(), po)


def test_entry_refuses_bad_arguments_and_an_empty_batch_is_ok():
    lens = _lens("rf50mm")
    pts = _points(2)
    x2, y2 = _disc(lens.entrance_pupil()[1] * 0.5, 64, seed=2)
    _, rec = _record(lens, pts, x2, y2)
    h, K = _lib.lib(), rec.n_surfaces
    rg = torch.zeros((4, 128), device=DEV)
    part = torch.empty((2, 1, 3), dtype=torch.float64, device=DEV)

    def call(trips, n_points, n_slices):
        return h.sdirt_trace2sensor_grad_points(rec.dev_lens.handle, (C.c_int32 * K)(*trips), 0, rec.d_sensor, dptr(rec.workspace),
                                                rec.ray.c_rays().ra, dptr(rg), 64, n_points, dptr(x2), dptr(y2),
                                                float(lens.entrance_pupil()[0]), dptr(part), n_slices, stream_ptr(lens.device))
    assert call(rec.trips, 2, 1) == 0
    assert call(rec.trips, 0, 7) == 0                                  # N = 0: nothing launched
    assert call(rec.trips, 2, 2) != 0                                  # n_slices must match
    assert call([-3 if t else 0 for t in rec.trips], 2, 1) == -2       # SDIRT_ERR_UNSUPPORTED: per-wave trips are not recorded


def _restated_call(lens, pts, recs, center, ks, r, normalize, GL, GR, x2, y2, xc, yc):
    """(dLoss/d(points), sum of |per-ray terms|) [N, 3] float64 of sum(GL L + GR R) by the restatement on the records of
    the call, CPU.  Every ray, primary and chief, has its own copy of the fp32 object point the kernels start from as
    a leaf; the summed leaves go through the pinhole scale (point_f64.chain), their magnitudes through its
    magnitudes; the pinhole centre of center=False is one more term per point."""
    prim = recs[-1]
    S, N = prim.ray.shape
    table = T.lens_table(lens, DEFAULT_WAVE)
    theta = lens.surface_parameters().double()
    p = pts.double().clone().requires_grad_()
    consts = (float(np.tan(lens.hfov)), float(lens.r_last), float(lens.sensor_size[1]), float(lens.sensor_size[0]))
    po = lens._points_to_object_now(pts).cpu().double()
    leaves = [po.unsqueeze(1).expand(N, S, 3).clone().requires_grad_()]
    ck = prim.workspace.view(prim.n_surfaces + 1, 6, S * N).cpu()
    ra = prim.ray.soa[6, :S * N].cpu()
    if center:
        chief = recs[0]
        Sc = chief.ray.shape[0]
        leaves.append(po.unsqueeze(1).expand(N, Sc, 3).clone().requires_grad_())
        ckc = chief.workspace.view(chief.n_surfaces + 1, 6, Sc * N).cpu()
        cen = P.centre(leaves[1], xc.cpu(), yc.cpu(), float(np.float32(lens.entrance_pupil(shrink_pupil=True)[0])), theta, table,
                       chief.trips, chief.d_sensor, chief.ray.soa[6, :Sc * N].cpu(), ckc)
    else:
        cen = torch.stack((p[:, 0] * consts[2] / 2, p[:, 1] * consts[3] / 2), -1)
    cen = T._at(prim.center.cpu().double(), cen)                     # the splat's decisions at the fp32 centres
    h, f, w = (torch.tensor(v, dtype=torch.float64) for v in DP[:3])
    L, R = P.psf_of_points(leaves[0], x2.cpu(), y2.cpu(), float(np.float32(lens.entrance_pupil()[0])), theta, table, prim.trips,
                           prim.d_sensor, cen, lens.pixel_size, ks, (h, f, w, r), ra, ck)
    if normalize:
        L, R = max_normalise(L), max_normalise(R)
    ((GL.cpu().double() * L).sum() + (GR.cpu().double() * R).sum()).backward()
    own = p.grad if p.grad is not None else torch.zeros_like(p)
    p0 = p.detach()
    want = P.chain(p0, sum(l.grad.sum(1) for l in leaves), *consts) + own
    mag = P.chain(p0, sum(l.grad.abs().sum(1) for l in leaves), *consts, absolute=True) + own.abs()
    return want, mag


class _Capture:
    """Keeps the TraceRecords of the calls made inside the block (chief bundle first, with center=True)."""

    def __init__(self, lens):
        self.lens, self.records = lens, []

    def __enter__(self):
        inner = self.lens._trace2sensor_recorded

        def wrapped(ray):
            rec = inner(ray)
            self.records.append(rec)
            return rec
        self.lens._trace2sensor_recorded = wrapped
        return self

    def __exit__(self, *exc):
        del self.lens.__dict__["_trace2sensor_recorded"]


def _call_samples(lens, spp, seed=11):
    x2, y2 = _disc(lens.entrance_pupil()[1], spp, seed)
    xc, yc = _disc(lens.entrance_pupil(shrink_pupil=True)[1], 2048, seed + 1)
    return (x2, y2), (xc, yc)


@pytest.mark.parametrize("name, ks, center, normalize, r", [
    ("rf50mm", 21, True, False, 0.5), ("rf50mm", 65, False, True, 0.65), ("rf35mm", 65, True, True, 0.65),
    ("rf35mm", 21, False, False, 0.5)])
def test_whole_call_matches_the_restatements_autograd(name, ks, center, normalize, r):
    lens = _lens(name)
    pts = _points(4, seed=7)
    pxy, cxy = _call_samples(lens, 2048)
    g = torch.Generator().manual_seed(3)
    GL, GR = (torch.randn((4, ks, ks), generator=g).to(DEV) for _ in range(2))
    p = pts.clone().requires_grad_()
    with _Capture(lens) as cap:
        L, R = lens.psf_lr(p, ks=ks, dp=(*DP[:3], r), center=center, normalize=normalize, pupil_xy=pxy,
                           center_pupil_xy=cxy if center else None, point_grad=True)
    ((GL * L).sum() + (GR * R).sum()).backward()
    assert len(cap.records) == (2 if center else 1)
    want, mag = _restated_call(lens, pts, cap.records, center, ks, r, normalize, GL, GR, *pxy, *cxy)
    got = p.grad.double()
    err = (got - want).abs() / mag
    print(f"{name} ks {ks} center {center} normalize {normalize} r {r}: grad {got.tolist()} "
          f"max |call - f64| / sum|terms| = {float(err.max()):.3e}, / |f64| = {float(((got - want).abs() / want.abs()).max()):.3e}")
    assert bool(torch.isfinite(got).all()) and float(got.abs().min()) > 0
    assert float(err.max()) <= TOL


def test_forward_bits_centres_and_the_pinhole_term():
    lens = _lens("rf50mm")
    pts, ks = _points(4, seed=8), 21
    pxy, cxy = _call_samples(lens, REPEATABLE_SPP)
    G = torch.randn((4, ks, ks), generator=torch.Generator().manual_seed(2)).to(DEV)
    for center in (True, False):
        kw = dict(ks=ks, center=center, pupil_xy=pxy, center_pupil_xy=cxy if center else None)
        p = pts.clone().requires_grad_()
        with _Capture(lens) as cap:
            L1, R1 = lens.psf_lr(p, dp=DP, point_grad=True, **kw)
        h = torch.tensor(DP[0], requires_grad=True)
        L2, R2 = lens.psf_lr(pts, dp=(h, *DP[1:]), **kw)
        assert torch.equal(L1.detach(), L2.detach()) and torch.equal(R1.detach(), R2.detach())
        (G * L1).sum().backward()
        g1 = p.grad.clone()
        # the same bits on every run
        p2 = pts.clone().requires_grad_()
        L3, _ = lens.psf_lr(p2, dp=DP, point_grad=True, **kw)
        (G * L3).sum().backward()
        assert torch.equal(g1, p2.grad) and torch.equal(L1.detach(), L3.detach())
        if center:
            # the staged chief centres are the fused pass's
            fused = torch.empty((4, 2), dtype=torch.float32, device=DEV)
            lens._chief_center(lens._points_to_object_now(pts), *cxy, lens.entrance_pupil(shrink_pupil=True)[0], fused)
            assert torch.equal(cap.records[1].center, fused)
            # without point_grad the points get nothing with center=True
            p3 = pts.clone().requires_grad_()
            h3 = torch.tensor(DP[0], requires_grad=True)
            L4, _ = lens.psf_lr(p3, dp=(h3, *DP[1:]), **kw)
            (G * L4).sum().backward()
            assert p3.grad is None
        else:
            # the pinhole-centre term of the default call plus the rays' term, computed separately
            p3 = pts.clone().requires_grad_()
            L4, _ = lens.psf_lr(p3, dp=DP, **kw)
            (G * L4).sum().backward()
            pin = p3.grad.double()
            assert bool((pin[:, 2] == 0).all()) and float(pin[:, :2].abs().min()) > 0
            rec = cap.records[0]
            # dLoss/d(raw L) of the max-normalised loss, by torch on the raw grid the call splatted
            Lr, _ = splat_autograd(rec.ray, lens.pixel_size, ks, rec.center, (*DP, "l"), lens.precision)
            Lr = Lr.detach().requires_grad_()
            Ln = Lr / (Lr.reshape(4, -1).max(dim=-1).values.reshape(4, 1, 1) + 1e-6)
            (G * Ln).sum().backward()
            rg = _ray_grad(rec, rec.center, lens.pixel_size, ks, Lr.grad.contiguous(), torch.zeros_like(Lr))
            smp = _samples(lens, *pxy)
            rays = TGm.points_chain(pts, TGm.points_bar(rec, rg, smp), smp).cpu()
            total = pin + rays
            err = (g1.double() - total).abs()
            assert bool((err <= 2.0 ** -23 * (pin.abs() + rays.abs())).all()), (g1, total)


def test_energy_alone_and_the_sum_of_the_three_outputs():
    lens = _lens("rf50mm")
    pts, ks = _points(4, seed=9), 21
    pxy, cxy = _call_samples(lens, REPEATABLE_SPP)
    g = torch.Generator().manual_seed(4)
    GL, GR = (torch.randn((4, ks, ks), generator=g).to(DEV) for _ in range(2))
    GE = torch.randn((4, 3), generator=g, dtype=torch.float64).to(DEV)
    smp = _samples(lens, *pxy)
    consts = (smp.tan_hfov, smp.r_last, smp.sensor_w, smp.sensor_h)

    def grad(use_l, use_r, use_e, center, point_grad=True):
        p = pts.clone().requires_grad_()
        with _Capture(lens) as cap:
            L, R, E = lens.psf_lr(p, ks=ks, dp=DP, normalize=False, center=center, pupil_xy=pxy,
                                  center_pupil_xy=cxy if center else None, energy=True, point_grad=point_grad)
        loss = 0
        if use_l:
            loss = loss + (GL * L).sum()
        if use_r:
            loss = loss + (GR * R).sum()
        if use_e:
            loss = loss + (GE * E).sum()
        loss.backward()
        return p.grad.double(), (cap.records[-1] if cap.records else None)

    def energy_ray_grad(rec):
        S, N = rec.ray.shape
        rg = torch.empty((4, S * N), dtype=torch.float32, device=DEV)
        dpp = _lib.DpParams(*DP)
        _lib.check(_lib.lib().sdirt_dp_energy_grad(rec.ray.c_rays(), S, N, C.byref(dpp), _flags(rec.precision),
                                                   dptr((GE / S).contiguous()), None, _slices(N, S), dptr(rg), 0,
                                                   stream_ptr(lens.device)))
        return rg
    # a loss on E alone, chief-ray centres: the entry on sdirt_dp_energy_grad's own ray_grad, bit for bit
    ge, rec = grad(False, False, True, center=True)
    want = TGm.points_chain(pts, TGm.points_bar(rec, energy_ray_grad(rec), smp), smp).to(torch.float32).cpu()
    assert float(ge.abs().max()) > 0 and torch.equal(ge.to(torch.float32), want)
    # L, R and E together against the three alone (pinhole centres: one bundle).  The rays' terms of the three meet in
    # fp32 in ray_grad before the ONE walk, where the three calls round each on its own: 2^-23 of the magnitudes, which
    # are the sums over the rays of the |per-ray terms| of the three (the restatement's) and the pinhole-centre terms
    ge, rec = grad(False, False, True, center=False)
    gl, _ = grad(True, False, False, center=False)
    gr, _ = grad(False, True, False, center=False)
    gall, _ = grad(True, True, True, center=False)
    zero = torch.zeros_like(GL)
    bars = [_restated_p_bar(lens, rec, rg, *pxy, smp.pupil_z)[1].cpu() for rg in (
        _ray_grad(rec, rec.center, lens.pixel_size, ks, GL, zero), _ray_grad(rec, rec.center, lens.pixel_size, ks, zero, GR),
        energy_ray_grad(rec))]
    mag = P.chain(pts.double(), sum(bars), *consts, absolute=True)
    for use in ((True, False), (False, True)):
        mag = mag + grad(*use, False, center=False, point_grad=False)[0].abs()
    err = (gall - (gl + gr + ge)).abs()
    print(f"L + R + E: max |together - sum| / sum|terms| = {float((err / mag).max()):.3e} (2^-23 = {2.0 ** -23:.3e})")
    assert float(gall.abs().min()) > 0 and bool((err <= 2.0 ** -23 * mag).all()), (gall, gl + gr + ge)


def test_other_gradients_do_not_change_and_psf_rgb_sums_its_wavelengths():
    lens = _lens("rf50mm")
    pts, ks = _points(4, seed=10), 21
    pxy, cxy = _call_samples(lens, REPEATABLE_SPP)
    G = torch.randn((4, ks, ks), generator=torch.Generator().manual_seed(5)).to(DEV)

    def grads(point_grad):
        theta = lens.surface_parameters().requires_grad_()
        glass = lens.glass_parameters().requires_grad_()
        s = torch.tensor(float(lens.d_sensor), requires_grad=True)
        p = pts.clone().requires_grad_(point_grad)
        L, R = lens.psf_lr(p, ks=ks, dp=DP, pupil_xy=pxy, center_pupil_xy=cxy, surface_params=theta, glass_params=glass,
                           d_sensor=s, point_grad=point_grad)
        ((G * L).sum() + (G * R).sum()).backward()
        return theta.grad, glass.grad, s.grad, p.grad, L.detach()
    a, b = grads(False), grads(True)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and torch.equal(a[4], b[4])
    assert a[3] is None and float(b[3].abs().min()) > 0
    # psf_rgb: the sum of the three wavelengths' gradients
    P3 = tuple(torch.stack([_call_samples(lens, REPEATABLE_SPP, seed=40 + i)[0][j] for i in range(3)]) for j in range(2))
    C3 = tuple(torch.stack([_call_samples(lens, REPEATABLE_SPP, seed=40 + i)[1][j] for i in range(3)]) for j in range(2))
    G3 = torch.randn((4, 3, ks, ks), generator=torch.Generator().manual_seed(6)).to(DEV)
    p = pts.clone().requires_grad_()
    rgb = lens.psf_rgb(p, ks=ks, param_list=[*DP, "l"], pupil_xy=P3, center_pupil_xy=C3, point_grad=True)
    # the addends of points.grad: per wavelength the rays' term (PointGradFunction) and the centre's (ChiefCentreFunction),
    # each the float64 result of trace_grad.points_chain, rounded to fp32 and added by autograd in fp32
    addends, chain = [], TGm.points_chain

    def recorded(*a):
        addends.append(chain(*a))
        return addends[-1]
    TGm.points_chain = recorded
    try:
        (G3 * rgb).sum().backward()
    finally:
        TGm.points_chain = chain
    assert len(addends) == 6
    mag = sum(a.abs() for a in addends).cpu()
    total = torch.zeros(4, 3, dtype=torch.float64)
    for i, wv in enumerate(WAVE_RGB):
        q = pts.clone().requires_grad_()
        L, _ = lens.psf_lr(q, ks=ks, wvln=wv, dp=DP, pupil_xy=(P3[0][i], P3[1][i]), center_pupil_xy=(C3[0][i], C3[1][i]),
                           point_grad=True)
        (G3[:, i] * L).sum().backward()
        total += q.grad.double()
    assert float(p.grad.abs().max()) > 0
    # the kernels are deterministic, so the six addends are the same bits on both sides; the rgb call adds them in fp32
    # in five additions, the three calls in one each: eight roundings, each at most 2^-24 of a partial sum that is at
    # most the sum of the |addends| (with center=True the rays' term and the centre's are each ~100 times their sum)
    err = (p.grad.double() - total).abs()
    print(f"psf_rgb: max |grad - sum of wavelengths| / sum|addends| = {float((err / mag).max()):.3e} (2^-21 = {2.0 ** -21:.3e})")
    assert bool((err <= 2.0 ** -21 * mag).all())


@pytest.mark.parametrize("xy", [(0.0, 0.0), (0.7, 0.5)])
def test_centre_jacobian_against_differences_of_the_fused_chief_centre(xy):
    """Independent of the restatement: d centre / d x from sdirt_chief_center at x +- 0.01 against the analytic Jacobian
    (a unit g_c back-propagated through ChiefCentreFunction).  The bar is the same quotient's error in float64 (the
    restatement's central difference at that step against its own autograd), times 2: tools/point_adam_f64.py prints
    it, 5.9e-7 of max |d c / d x| on axis and 1.6e-6 at (0.7, 0.5) (JAC_ERR there).

    The quotient divides by the step the entry was actually given: sdirt_chief_center takes fp32 object points, and
    0.71 - 0.69 in fp32 is 0.02 (1 - 9.5e-7) before the pinhole scale rounds once more; over the nominal 0.02 the
    quotient at (0.7, 0.5) came out 7.4e-5 low (bar 5.6e-5), 1.7e-5 of it that rounding of the step alone.

    Measured on MI355X.  On axis: quotient 17.635191, analytic 17.635183, |difference| 7.4e-6 against a bar of 2.09e-5.
    At (0.7, 0.5): quotient 17.631388, analytic 17.631414 (the float64 restatement's own Jacobian is 17.631412),
    |difference| 2.6e-5 against a bar of 5.61e-5; the float64 quotient's own truncation error there is 2.8e-5."""
    import point_adam_f64 as A
    lens = _lens("rf50mm")
    step = A.JAC_STEP
    pts = torch.tensor([[xy[0], xy[1], -1500.0]])
    xc, yc = (t.to(DEV) for t in A.problem(lens.entrance_pupil()[1])[2])              # the tool's chief-ray samples
    pz = lens.entrance_pupil(shrink_pupil=True)[0]

    def fused(x):
        q = pts.clone()
        q[0, 0] = x
        out = torch.empty((1, 2), dtype=torch.float32, device=DEV)
        po = lens._points_to_object_now(q)
        lens._chief_center(po, xc, yc, pz, out)
        return out.cpu().double()[0], float(po[0, 0])
    (c_hi, x_hi), (c_lo, x_lo) = fused(xy[0] + step), fused(xy[0] - step)
    # the step the entry was given: sdirt_chief_center takes the fp32 object points, whose x differ by x_hi - x_lo, not
    # by 2 step d(point_obj.x)/dx exactly (0.71 and 0.69 are no fp32 numbers, and the pinhole scale rounds once more)
    dpo_dx = -float(pts[0, 2]) * float(np.tan(lens.hfov)) / float(lens.r_last) * float(lens.sensor_size[1]) / 2
    quot = (c_hi - c_lo) / (x_hi - x_lo) * dpo_dx
    print(f"xy {xy}: step in point_obj.x {x_hi - x_lo:.9e}, nominal {2 * step * dpo_dx:.9e}; quotient over the nominal step "
          f"{((c_hi - c_lo) / (2 * step)).tolist()}")
    jac = []
    for comp in range(2):
        p = pts.clone().requires_grad_()
        cen = torch.empty((1, 2), dtype=torch.float32, device=DEV)
        rec = lens._chief_center_recorded(lens._points_to_object_now(pts), xc, yc, pz, cen)
        c = TGm.ChiefCentreFunction.apply(p, cen, rec, _samples(lens, xc, yc, shrink=True))
        c[0, comp].backward()
        jac.append(float(p.grad[0, 0]))
    jac = torch.tensor(jac, dtype=torch.float64)
    bar = 2 * A.JAC_ERR[xy] * float(jac.abs().max())
    print(f"xy {xy}: quotient {quot.tolist()} analytic {jac.tolist()} bar {bar:.3e}")
    assert float(jac.abs().max()) > 1 and float((quot - jac).abs().max()) <= bar


def test_depth_by_descent():
    """tools/point_adam_f64.py's problem: rf50mm with the sensor where refocus(-1000) puts it, four points (on axis,
    mid-field, a corner, one far behind the focus plane), 4096 fixed pupil samples, ks 31, chief-ray centres; targets
    the model's own sum-normalised L and R at the true depths, the depths start 8 % off, Adam on the depths.  In
    float64 on the CPU with the restatement the loss falls to 6.04e-4 of its first value and max |z / truth - 1| to
    4.82e-3 (RATIO, LEFT in the tool); the asserts leave a margin of 1.4."""
    import point_adam_f64 as A
    lens = _lens("rf50mm")
    pts, pxy, cxy = A.problem(lens.entrance_pupil()[1])
    pxy, cxy = tuple(t.to(DEV) for t in pxy), tuple(t.to(DEV) for t in cxy)
    kw = dict(ks=A.KS, dp=A.DP, normalize=False, pupil_xy=pxy, center_pupil_xy=cxy, d_sensor=A.D_SENSOR)

    def sum_normalised(L, R):
        return L / L.sum((-1, -2), keepdim=True), R / R.sum((-1, -2), keepdim=True)
    with torch.no_grad():
        tL, tR = sum_normalised(*lens.psf_lr(pts, **kw))
    z0 = pts[:, 2] * A.START
    zs = [z.clone().requires_grad_() for z in z0]
    opt = torch.optim.Adam([{"params": [z], "lr": lr} for z, lr in zip(zs, A.step_lengths(z0))])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 - k / A.STEPS)
    losses = []
    for _ in range(A.STEPS):
        p = torch.cat((pts[:, :2], torch.stack(zs).unsqueeze(1)), 1)
        L, R = sum_normalised(*lens.psf_lr(p, point_grad=True, **kw))
        loss = ((L - tL) ** 2).sum() + ((R - tR) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss))
    z = torch.stack(zs).detach()
    left = float((z / pts[:, 2] - 1).abs().max())
    print("losses", ["%.3e" % v for v in losses[::5]], f"ratio {losses[-1] / losses[0]:.4e} left {left:.4e}")
    assert all(b < a for a, b in zip(losses[:10], losses[1:11]))
    assert losses[-1] / losses[0] <= 1.4 * A.RATIO
    assert left <= 1.4 * A.LEFT
