"""Gradients of dual-pixel PSFs in the glass (n, V of every medium) on the GPU: psf_lr / psf_diff / psf_rgb / psf_volume
with `glass_params=` (sdirt_trace2sensor_record, sdirt_forward_integral_grad_rays, sdirt_trace2sensor_grad_eta;
DESIGN.md 7i).  Structured like test_gpu_trace_grad.py.

B. The eta column against the float64 restatement (tests/glass_f64.py on tests/trace_f64.py) on the kernel's own fp32
   checkpoints, trip tables and per-ray upstream gradients, with per-ray eta leaves taken to (n, V) by the Jacobian of eta
   in the glass: per owned (medium, column) |kernel - float64| <= TOL * (sum |per-ray terms| + floor).  Shapes: a tail
   (rays no multiple of 64 or 256), vignetted corners, more rays than the launch has threads, a refracting plane.
C. The ABI column directly, and the properties of the Python layer.
D. The sum over wavelengths (psf_rgb, the chromatic volume, the render) and a one-parameter fit by Adam.

TOL = 2 * max(spread, 1e-4) is the rule of DESIGN.md 7d/7f; the spread of the reference's own fp32-against-float64
autograd in the same normalised form is at most 5.4e-6 on its corner cases at the three wavelengths
(tools/gen_glass_grad.py), so TOL is the rule's floor, 2e-4."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

import glass_f64 as G
from conftest import ROOT, load_state, make_lens
from test_gpu_trace_grad import _abi, _Capture, _points, _pupil, _ray_grad
from test_gpu_trace_grad import _restated as _restated_theta

sys.path.insert(0, os.path.join(ROOT, "tools"))

from sdirt_amd import _lib
from sdirt_amd.basics import WAVE_RGB, dptr, stream_ptr
from sdirt_amd.trace_grad import N_COLUMNS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
TOL = 2e-4
REPEATABLE_SPP = 1000           # (test_gpu_trace_grad.py: below the spp cut the forward's grids repeat bit for bit)


def _lens(name):
    return make_lens(name, DEV, load_state(name))


def _eta_jacobian(lens, wvln):
    """d eta_k / d glass[j, c], [K, K + 1, 2] float64, from the restatement's own formula."""
    return torch.autograd.functional.jacobian(lambda g: G.eta(g, lens, wvln), lens.glass_parameters())


def _restated(lens, rec, ray_grad, wvln, chunk=1 << 16):
    """(gradient, sum of |per-ray terms|) [K + 1, 2] float64 in the glass, and per surface the sum of |per-ray eta terms|
    [K], of sum_rays ray_grad . (o.x, o.y, d.x, d.z) at the sensor: the float64 restatement on the kernel's checkpoints
    with one eta leaf per ray and surface, on the GPU in chunks of rays."""
    K, M = rec.n_surfaces, rec.ray.numel
    ws = rec.workspace.view(K + 1, 6, M)
    ra = rec.ray.soa[6, :M]
    idx = torch.nonzero((ra != 0) & (ray_grad != 0).any(0)).reshape(-1)
    theta = lens.surface_parameters().double().to(DEV)
    e0 = G.eta(lens.glass_parameters(), lens, wvln).to(DEV)
    J = _eta_jacobian(lens, wvln).to(DEV)
    tot = torch.zeros((K + 1, 2), dtype=torch.float64, device=DEV)
    mag, eta_mag = torch.zeros_like(tot), torch.zeros(K, dtype=torch.float64, device=DEV)
    for a in range(0, idx.numel(), chunk):
        ii = idx[a:a + chunk]
        ck = ws[:, :, ii]
        leaves = [e0[k].expand(ii.numel(), 1).clone().requires_grad_() for k in range(K)]
        o, d = ck[0, :3].t().double(), ck[0, 3:].t().double()
        so, sd = G.trace_f64(o, d, theta, G.glass_table(lens, wvln, leaves), rec.trips, rec.d_sensor, checkpoints=ck)
        g = ray_grad[:, ii].double()
        (g[0] * so[:, 0] + g[1] * so[:, 1] + g[2] * sd[:, 0] + g[3] * sd[:, 2]).sum().backward()
        per_ray = torch.stack([l.grad.reshape(-1) if l.grad is not None else torch.zeros_like(g[0]) for l in leaves], -1)
        terms = torch.einsum("mk,kjc->mjc", per_ray, J)
        tot += terms.sum(0)
        mag += terms.abs().sum(0)
        eta_mag += per_ray.abs().sum(0)
    return tot.cpu(), mag.cpu(), eta_mag.cpu(), int(idx.numel())


def _kernel_grad(lens, pts, ks, pxy, cxy, GL, GR, wvln):
    glass = lens.glass_parameters().requires_grad_()
    with _Capture(lens) as cap:
        L, R = lens.psf_lr(pts, ks=ks, wvln=wvln, dp=DP, normalize=False, pupil_xy=pxy, center_pupil_xy=cxy, glass_params=glass)
    ((GL * L).sum() + (GR * R).sum()).backward()
    assert glass.grad.dtype == torch.float64 and glass.grad.device.type == "cpu"
    return glass.grad, cap.records[0]


def _check_against_restatement(lens, pts, ks, spp, wvln, label, min_dead=None):
    pxy, cxy = _pupil(lens, pts, spp)
    N = pts.shape[0]
    g = torch.Generator().manual_seed(3)
    GL, GR = (torch.randn((N, ks, ks), generator=g).to(DEV) for _ in range(2))
    got, rec = _kernel_grad(lens, pts, ks, pxy, cxy, GL, GR, wvln)
    rg = _ray_grad(rec, rec.center, lens.pixel_size, ks, GL, GR)
    assert bool(torch.isfinite(rg).all())
    want, mag, eta_mag, n_live = _restated(lens, rec, rg, wvln)
    own = lens.glass_owned()
    dead = float((rec.ray.soa[6, :rec.ray.numel] == 0).float().mean())
    # 1e-12 of the column's largest sum stands in for a sum of float64 rounding noise (as test_gpu_trace_grad.py's floor)
    floor = 1e-12 * mag.max(0, keepdim=True).values
    err = ((got - want).abs() / (mag + floor).clamp_min(1e-300))[own]
    print(f"{label}: rays {rec.ray.numel} live-in-window {n_live} dead {dead:.3f} trips {rec.trips} "
          f"max |kernel - f64| / sum|terms| = {float(err.max()):.3e}")
    assert bool(torch.isfinite(got).all()) and n_live > 0
    assert bool((got[~own] == 0).all())
    assert bool((mag[own] > 0).all()) and bool((got[own] != 0).all())
    if min_dead is not None:
        assert dead >= min_dead, dead
    assert float(err.max()) <= TOL
    return got, rec, eta_mag


@pytest.mark.parametrize("name, precision, ks, wvln", [("rf50mm", "lean", 21, 0.486), ("rf35mm", "ieee", 33, 0.656)])
def test_eta_column_on_a_batch_with_a_tail(name, precision, ks, wvln):
    """5 x 1999 = 9995 rays: no multiple of 64 or 256, so the last workgroup has idle lanes and idle waves."""
    lens = _lens(name)
    lens.precision = precision
    _check_against_restatement(lens, _points(5), ks, 1999, wvln, f"{name} {precision} ks{ks} {wvln} um 5x1999")


@pytest.mark.parametrize("name", ["rf50mm", "rf35mm"])
def test_eta_column_on_a_vignetted_batch(name):
    """The eight points of test_adjoint_kernel_on_a_vignetted_batch (the reference's own trace loses 5.1 % of rf50mm's rays
    and 10.2 % of rf35mm's on them), 2048 samples."""
    lens = _lens(name)
    f = {"rf50mm": 0.98, "rf35mm": 1.08}[name]
    pts = torch.tensor([[f, f, -300.0], [-f, f, -20000.0], [f, -f, -500.0], [-f, -f, -300.0],
                        [0.0, 0.98, -300.0], [0.98, 0.0, -20000.0], [0.0, 0.0, -1500.0], [0.7, 0.7, -300.0]])
    _check_against_restatement(lens, pts, 21, 2048, 0.589, f"{name} vignetted", min_dead=0.03)


def test_eta_column_with_more_rays_than_the_launch_has_threads():
    """ceil(8 n_cus 256 / 8192) + 1 points x 8192 samples (65 x 8192 on 256 CUs, one point more than the 8 n_cus workgroups of
    256 threads hold): workgroups stride the grid."""
    lens = _lens("rf50mm")
    ncu = int(torch.cuda.get_device_properties(DEV).multi_processor_count)
    n = math.ceil(8 * ncu * 256 / 8192) + 1
    _, rec, _ = _check_against_restatement(lens, _points(n), 21, 8192, 0.589, f"rf50mm grid stride {n}x8192")
    assert rec.ray.numel > 8 * ncu * 256


def test_eta_column_of_a_refracting_plane(tmp_path):
    """rf50mm behind a 1 mm cover glass (no shipped lens has a refracting plane): both planes own their eta column with a
    non-zero magnitude, the stop's stays exactly 0."""
    lens = G.cover_glass_lens(tmp_path, DEV)
    K = len(lens.surfaces)
    assert [s.kind for s in lens.surfaces[-2:]] == [_lib.KIND_PLANE] * 2 and bool(lens.glass_owned()[K - 1])
    got, rec, eta_mag = _check_against_restatement(lens, _points(4), 21, 999, 0.486, "rf50mm + cover glass 4x999")
    assert float(eta_mag[K - 2]) > 0 and float(eta_mag[K - 1]) > 0 and float(eta_mag[lens.aper_idx]) == 0
    assert float(got[K - 1, 0]) != 0 and float(got[K - 1, 1]) != 0
    partial = _abi(rec, _upstream(lens, rec, 21), "sdirt_trace2sensor_grad_eta").sum(0)
    assert float(partial[K - 2, N_COLUMNS]) != 0 and float(partial[K - 1, N_COLUMNS]) != 0
    assert float(partial[lens.aper_idx, N_COLUMNS]) == 0


def _upstream(lens, rec, ks, seed=3):
    N = rec.ray.shape[1]
    g = torch.Generator().manual_seed(seed)
    GL, GR = (torch.randn((N, ks, ks), generator=g).to(DEV) for _ in range(2))
    return _ray_grad(rec, rec.center, lens.pixel_size, ks, GL, GR)


def test_abi_eta_entry_returns_the_old_columns_and_an_exact_zero_on_the_stop():
    lens = _lens("rf50mm")
    pts, ks = _points(6), 21
    pxy, cxy = _pupil(lens, pts, 1500)
    glass = lens.glass_parameters().requires_grad_()
    with _Capture(lens) as cap:
        lens.psf_lr(pts, ks=ks, dp=DP, normalize=False, pupil_xy=pxy, center_pupil_xy=cxy, glass_params=glass)
    rec = cap.records[0]
    rg = _upstream(lens, rec, ks)
    old = _abi(rec, rg, "sdirt_trace2sensor_grad")
    new = _abi(rec, rg, "sdirt_trace2sensor_grad_eta")
    again = _abi(rec, rg, "sdirt_trace2sensor_grad_eta")
    assert new.shape == (old.shape[0], old.shape[1], N_COLUMNS + 1) and bool(torch.isfinite(new).all())
    assert torch.equal(new, again)                                             # the same bits every run
    _, mag, _ = _restated_theta(lens, rec, rg)
    diff = (new[..., :N_COLUMNS].sum(0) - old.sum(0)).abs().cpu()
    print(f"columns 0-10, eta entry against the old one: max |diff| / sum|terms| = {float((diff / mag.clamp_min(1e-300)).max()):.3e}")
    assert bool((diff <= 1e-12 * mag).all())
    # ... and bit for bit, workgroup by workgroup: the two entries are one kernel body, the same float64
    # operations in the same order
    assert torch.equal(new[..., :N_COLUMNS], old)
    eta_col = new[..., N_COLUMNS]
    assert bool((eta_col[:, lens.aper_idx] == 0).all())
    others = [k for k in range(len(lens.surfaces)) if k != lens.aper_idx]
    assert bool((eta_col.sum(0)[others] != 0).all())
    # the argument checks are the old entry's
    h = _lib.lib()
    K, M = rec.n_surfaces, rec.ray.numel
    args = lambda trips, nwg: (rec.dev_lens.handle, (C.c_int32 * K)(*trips), 0, rec.d_sensor, dptr(rec.workspace),
                               rec.ray.c_rays().ra, dptr(rg), M, dptr(new), nwg, stream_ptr(torch.device(DEV)))
    assert h.sdirt_trace2sensor_grad_eta(*args(rec.trips, new.shape[0] + 1)) == -1            # SDIRT_ERR_INVALID_ARGUMENT
    assert h.sdirt_trace2sensor_grad_eta(*args([-10] * K, new.shape[0])) == -2                       # SDIRT_ERR_UNSUPPORTED
    assert h.sdirt_trace2sensor_grad_eta(None, *args(rec.trips, new.shape[0])[1:]) == -1


def test_forward_bits_determinism_zero_rows_other_gradients_and_state():
    lens = _lens("rf50mm")
    pts, ks, spp = _points(16), 33, REPEATABLE_SPP
    pxy, cxy = _pupil(lens, pts, spp)
    kw = dict(ks=ks, wvln=0.486, pupil_xy=pxy, center_pupil_xy=cxy)
    G_ = torch.randn((16, ks, ks), generator=torch.Generator().manual_seed(2)).to(DEV)
    own = lens.glass_owned()
    with torch.no_grad():
        before = lens.psf_lr(pts, dp=DP, **kw)
    mats = [(m.n, m.V, m.A, m.B, m.name) for s in lens.surfaces for m in (s.mat1, s.mat2)]
    state = (lens.glass_parameters(), dict(lens._dev), dict(lens._pupil_cache), lens.trips, dict(lens.trips.cache))
    glass0 = lens.glass_parameters()
    glass0[1, 0] += 1.5e-3
    glass0[4, 1] *= 0.98
    theta0 = lens.surface_parameters()
    theta0[2, 0] += 0.02
    s0 = float(lens.d_sensor) + 0.05

    def grads(want_h=False, want_theta=False, want_s=False, want_glass=False):
        h = torch.tensor(DP[0], requires_grad=want_h)
        theta = theta0.clone().requires_grad_(want_theta)
        s = torch.tensor(s0, dtype=torch.float64, requires_grad=want_s)
        glass = glass0.clone().requires_grad_(want_glass)
        target = lens                                   # all four: the lens is borrowed
        if not (want_h and want_theta and want_s and want_glass):
            target = _lens("rf50mm").set_surface_parameters(theta0).set_glass_parameters(glass0)      # permanently that lens
        L, R = target.psf_lr(pts, dp=(h, *DP[1:]), d_sensor=s if want_s else s0,
                             surface_params=theta if want_theta else None, glass_params=glass if want_glass else None, **kw)
        (G_ * L).sum().backward()
        return L.detach(), R.detach(), h.grad, theta.grad, s.grad, glass.grad
    L1, R1, h1, t1, s1, g1 = grads(True, True, True, True)
    L2, R2, h2, t2, s2, g2 = grads(True, True, True, True)
    assert torch.equal(L1, L2) and torch.equal(R1, R2)
    assert torch.equal(h1, h2) and torch.equal(t1, t2) and torch.equal(s1, s2) and torch.equal(g1, g2)   # the same bits every run
    assert g1.shape == glass0.shape and g1.dtype == torch.float64
    assert bool(torch.isfinite(g1).all()) and bool((g1[own] != 0).all()) and bool((g1[~own] == 0).all())
    # ... left the lens as it was: materials, records, device tables, pupils, planner
    assert [(m.n, m.V, m.A, m.B, m.name) for s in lens.surfaces for m in (s.mat1, s.mat2)] == mats
    assert torch.equal(lens.glass_parameters(), state[0])
    assert lens._dev == state[1] and lens._pupil_cache == state[2] and lens.trips is state[3]
    assert all(np.array_equal(v, lens.trips.cache[k]) for k, v in state[4].items()) and set(state[4]) == set(lens.trips.cache)
    with torch.no_grad():
        after = lens.psf_lr(pts, dp=DP, **kw)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # each gradient equals the call that asks for it alone (on a lens permanently set to the other values: the same
    # staged chain, so the forward is bit-equal too), within 2^-23 of its own magnitude, which is at most sum |terms|
    for i, name in enumerate(("h", "theta", "d_sensor", "glass")):
        flags = [j == i for j in range(4)]
        alone = grads(*flags)
        assert torch.equal(alone[0], L1) and torch.equal(alone[1], R1), name
        a, b = alone[2 + i].double(), (h1, t1, s1, g1)[i].double()
        print(f"{name}.grad, one call for all four against its own call: max |diff| / |grad| = "
              f"{float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()):.3e}")
        # (an entry that vanishes identically, the stop's d, is float64 rounding noise: 1e-12 of the largest entry stands in)
        assert bool(((a - b).abs() <= 2.0 ** -23 * (torch.maximum(a.abs(), b.abs()) + 1e-12 * b.abs().max())).all()), name
    # refused as for surface_params
    req = lambda: glass0.clone().requires_grad_()
    with pytest.raises(ValueError):
        lens.psf_lr(pts, dp=DP, glass_params=req(), defer=True, **kw)
    with pytest.raises(ValueError):
        lens.psf_lr(pts, dp=DP, glass_params=req(), out=(torch.empty((16, ks, ks), device=DEV), torch.empty((16, ks, ks), device=DEV)), **kw)
    with pytest.raises(ValueError):
        lens.psf_lr(pts, dp=DP, glass_params=req(), center_out=torch.empty((16, 2), device=DEV), **kw)
    lens.trip_policy = "adaptive"
    with pytest.raises(ValueError):
        lens.psf_lr(pts, dp=DP, glass_params=req(), **kw)
    lens.trip_policy = "reference"
    assert [(m.n, m.V, m.A, m.B, m.name) for s in lens.surfaces for m in (s.mat1, s.mat2)] == mats
    # glass_params without a gradient is set_glass_parameters + the ordinary call
    third, other = _lens("rf50mm"), _lens("rf50mm")
    other.set_glass_parameters(glass0)
    with torch.no_grad():
        a = third.psf_lr(pts, dp=DP, glass_params=glass0, **kw)
        b = other.psf_lr(pts, dp=DP, **kw)
    assert torch.equal(third.glass_parameters(), glass0) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], before[0])


def test_surface_params_alone_still_goes_through_the_old_entry_bit_for_bit():
    lens = _lens("rf50mm")
    pts, ks = _points(8), 21
    pxy, cxy = _pupil(lens, pts, REPEATABLE_SPP)
    g = torch.Generator().manual_seed(3)
    GL, GR = (torch.randn((8, ks, ks), generator=g).to(DEV) for _ in range(2))
    theta = lens.surface_parameters().requires_grad_()
    with _Capture(lens) as cap:
        L, R = lens.psf_lr(pts, ks=ks, dp=DP, normalize=False, pupil_xy=pxy, center_pupil_xy=cxy, surface_params=theta)
    ((GL * L).sum() + (GR * R).sum()).backward()
    rec = cap.records[0]
    old = _abi(rec, _ray_grad(rec, rec.center, lens.pixel_size, ks, GL, GR), "sdirt_trace2sensor_grad")
    assert torch.equal(theta.grad, old.sum(0).to("cpu", torch.float32))


def _per_wavelength_pupils(lens, pts, spp):
    P, Pc = [], []
    for i in range(3):
        pxy, cxy = _pupil(lens, pts, spp, seed=20 + i)
        P.append(pxy); Pc.append(cxy)
    return ((torch.stack([p[0] for p in P]), torch.stack([p[1] for p in P])),
            (torch.stack([p[0] for p in Pc]), torch.stack([p[1] for p in Pc])))


def test_psf_rgb_glass_gradient_is_the_sum_of_its_wavelengths():
    lens = _lens("rf50mm")
    pts, ks = _points(6), 21
    P, Pc = _per_wavelength_pupils(lens, pts, REPEATABLE_SPP)
    G_ = torch.randn((6, 3, ks, ks), generator=torch.Generator().manual_seed(8)).to(DEV)
    glass = lens.glass_parameters().requires_grad_()
    rgb = lens.psf_rgb(pts, ks=ks, param_list=[*DP, "l"], pupil_xy=P, center_pupil_xy=Pc, glass_params=glass)
    (G_ * rgb).sum().backward()
    total = torch.zeros_like(glass.grad)
    for i in reversed(range(3)):                    # autograd runs the branch made last first, and adds in that order
        gl = lens.glass_parameters().requires_grad_()
        L, _ = lens.psf_lr(pts, ks=ks, wvln=WAVE_RGB[i], dp=DP, pupil_xy=(P[0][i], P[1][i]), center_pupil_xy=(Pc[0][i], Pc[1][i]),
                           glass_params=gl)
        (G_[:, i] * L).sum().backward()
        total += gl.grad
    own = lens.glass_owned()
    assert glass.grad.dtype == torch.float64 and torch.equal(glass.grad, total)          # float64 all the way: bit for bit
    assert bool((glass.grad[own] != 0).all()) and bool((glass.grad[~own] == 0).all())     # V of every owned medium too


def test_chromatic_volume_glass_gradient_is_the_sum_and_reaches_an_image_loss():
    lens = _lens("rf50mm")
    ks, H, W = 21, 32, 48
    torch.manual_seed(3)
    with torch.no_grad():
        lens.psf_lr(torch.tensor([[0.0, 0.0, -1500.0]]), ks=ks, spp=REPEATABLE_SPP)
    pupil = tuple(t.clone() for t in lens.last_pupil_points)
    kw = dict(grid=(4, 4), z=2, ks=ks, spp=REPEATABLE_SPP, pupil_xy=pupil[:2], center_pupil_xy=pupil[2:])
    Gv = torch.randn((3, 2, 4, 4, 2, ks, ks), generator=torch.Generator().manual_seed(5)).to(DEV)
    glass = lens.glass_parameters().requires_grad_()
    vol = lens.psf_volume(wvln=WAVE_RGB, glass_params=glass, **kw)
    assert vol.psf.shape == Gv.shape
    (Gv * vol.psf).sum().backward()
    total = torch.zeros_like(glass.grad)
    for i in reversed(range(3)):
        gl = lens.glass_parameters().requires_grad_()
        one = lens.psf_volume(wvln=WAVE_RGB[i], glass_params=gl, **kw)
        (Gv[i] * one.psf).sum().backward()
        total += gl.grad
    own = lens.glass_owned()
    assert torch.equal(glass.grad, total)
    assert bool((glass.grad[own] != 0).all()) and bool((glass.grad[~own] == 0).all())
    # through the render of a 32 x 48 RGB frame an image loss reaches the glass
    gen = torch.Generator().manual_seed(4)
    img = torch.rand((1, 3, H, W), generator=gen).to(DEV)
    z = torch.rand((1, H, W), generator=gen).to(DEV)
    gl = lens.glass_parameters().requires_grad_()
    out = lens.psf_volume(wvln=WAVE_RGB, glass_params=gl, **kw).render(img, z)
    ((out - torch.roll(out.detach(), 1, -1)) ** 2).sum().backward()
    assert bool(torch.isfinite(gl.grad).all()) and bool((gl.grad[own] != 0).all()) and bool((gl.grad[~own] == 0).all())


def test_adam_recovers_a_perturbed_index():
    """PSFs of the true lens as the target; n of rf50mm's first element starts 2e-3 too high.  The problem is
    tools/adam_glass_f64.py's, which runs it in float64 on the CPU with the restatement: there the loss falls monotonically
    to 0.0979 of its first value in 12 steps and |n - truth| to 0.2625 of where it starts.  The bounds leave 7f's margin
    of 1.4 on each for fp32 rays, Monte-Carlo grids and the pupil plane the library recomputes for every glass: 0.137 and
    0.3675."""
    import adam_glass_f64 as A
    lens = _lens("rf50mm")
    pts, pxy = A.problem(lens.entrance_pupil()[1])
    kw = dict(ks=A.KS, dp=A.DP, center=False, pupil_xy=pxy, wvln=A.WVLN)
    truth = lens.glass_parameters()
    assert bool(lens.glass_owned()[A.MEDIUM])
    with torch.no_grad():
        tL, tR = lens.psf_lr(pts, **kw)
    n_par = (truth[A.MEDIUM, 0] + A.N_OFF).clone().requires_grad_()
    opt = torch.optim.Adam([n_par], lr=A.LR_N)
    losses = []
    for _ in range(A.STEPS):
        glass = truth.clone()
        glass[A.MEDIUM, 0] = n_par
        L, R = lens.psf_lr(pts, glass_params=glass, **kw)
        loss = ((L - tL) ** 2).mean() + ((R - tR) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    n_left = abs(float(n_par) - float(truth[A.MEDIUM, 0])) / A.N_OFF
    print("losses", ["%.3e" % v for v in losses], f"ratio {losses[-1] / losses[0]:.4f} n left {n_left:.4f}")
    assert all(b < a for a, b in zip(losses[:5], losses[1:6]))                 # falls monotonically over the first steps
    assert float(n_par) < float(truth[A.MEDIUM, 0]) + A.N_OFF                  # toward the truth
    assert losses[-1] / losses[0] <= 0.137
    assert n_left <= 0.3675
    assert torch.equal(lens.glass_parameters(), truth)
