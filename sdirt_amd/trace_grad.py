"""The backward pass of the staged trace as an autograd op: surface parameters theta [K, 3 + MAX_AI] (columns d, c, k,
ai2, ai4, ...) get the gradient the reference's graph gives them (deeplens/surfaces.py:523-679 under autograd), and the
glass [K + 1, 2] (columns n, V of every medium) gets its own through eta_k = n_k(lambda) / n_k+1(lambda).

The forward of a psf call with `surface_params=` or `glass_params=` is the staged chain with a RECORDING trace
(sdirt_trace2sensor_record: every ray's (o, d) on entry to each surface); the raw grids come from
monte_carlo.SplatFunction as in every other differentiable call.  SurfaceGradFunction sits behind those grids as an
identity: its backward receives dLoss/d(raw grids), turns it into dLoss/d(sensor-plane rays)
(sdirt_forward_integral_grad_rays) and walks the recorded trace backwards ONCE (sdirt_trace2sensor_grad; with a glass,
sdirt_trace2sensor_grad_eta, whose extra column is dLoss/d eta); the grids' gradients pass through unchanged to
SplatFunction, so h, f, w and the pinhole centres get theirs in the same backward.  eta is a float64 torch function of the
glass (glass_eta), so torch's own autograd takes dLoss/d eta on to (n, V).
"""
import ctypes as C

import torch

from . import _lib
from .basics import Material, dptr, stream_ptr
from .monte_carlo import _flags, grad_slices, n_cus

N_COLUMNS = 3 + _lib.MAX_AI


def glass_eta(glass, owned, constants, wvln):
    """eta [K] = n_k(wvln) / n_k+1(wvln), float64, as a torch function of glass [K + 1, 2] (columns n, V).  An owned
    medium j (owned[j]) is the Cauchy glass of its row, n(lambda) = A + B / lambda_nm^2 with Material.nV_to_AB's A and B
    in Material.ior's order of operations (basics.py:336-338, 355-362): the values are the n1 / n2 the device table is
    built from.  Every other medium is the constant constants[j] (its Material.ior(wvln)) without a gradient."""
    wv = wvln if wvln < 10 else wvln * 1e-3
    g = glass.to(torch.float64)
    n, V = g[:, 0], g[:, 1]
    own = torch.as_tensor(owned, dtype=torch.bool)
    V = torch.where(own, V, torch.ones_like(V))                       # (a constant's V may be 0: never divided by)
    A, B = Material.nV_to_AB(n, V)
    ior = torch.where(own, A + B / (wv * 1e3) ** 2, torch.as_tensor(constants, dtype=torch.float64))
    return ior[:-1] / ior[1:]


class TraceRecord:
    """What the backward needs of one recorded trace: the device lens (kept alive), the trip table and math policy of the
    recording launch, the sensor plane, the checkpoints and the sensor-plane bundle."""

    def __init__(self, dev_lens, trips, precision, d_sensor, workspace, ray, n_surfaces):
        self.dev_lens, self.trips, self.precision, self.d_sensor = dev_lens, [int(t) for t in trips], precision, float(d_sensor)
        self.workspace, self.ray, self.n_surfaces = workspace, ray, int(n_surfaces)
        self.center = None          # the [N, 2] centres the splat used (set by the psf call)


class PointSamples:
    """What takes a recorded bundle's adjoint on to the caller's points: the pupil sample points the bundle was sampled
    with (x2, y2 [spp] fp32 on the device, pupil_z) and the constants of the pinhole scale (optics.py:956-960)."""

    def __init__(self, x2, y2, pupil_z, tan_hfov, r_last, sensor_w, sensor_h):
        self.x2, self.y2, self.pupil_z = x2, y2, float(pupil_z)
        self.tan_hfov, self.r_last, self.sensor_w, self.sensor_h = float(tan_hfov), float(r_last), float(sensor_w), float(sensor_h)


def _identity_outputs(ctx, lg, rg, energy):
    """The forward of an identity behind the raw grids (and, with `energy`, the sums)."""
    ctx.has_energy = energy is not None
    if energy is None:
        return lg.clone(), rg.clone()
    ctx.set_materialize_grads(False)        # an output the loss does not use arrives as None, not as zeros
    return lg.clone(), rg.clone(), energy.clone()


def ray_adjoint(rec, center, geom, dp, gl, gr, ge, wanted=True):
    """dLoss/d(sensor-plane rays) of the record `rec` from dLoss/d(raw grids) gl, gr and dLoss/d(sums) ge (`ge` as
    backward's *args; each may be None): sdirt_forward_integral_grad_rays writes ray_grad [4, M] fp32 unless only the
    sums bring a gradient, and sdirt_dp_energy_grad adds the sums' terms to it (accumulate = 1) or writes it alone
    (accumulate = 0).  -> (ray_grad, gl, gr, ge), the three in the types the library takes; ray_grad is None, and
    nothing is launched, when it is not `wanted`."""
    ray, (ps, ks) = rec.ray, geom
    S, N = ray.shape
    dev = ray.device
    h, st = _lib.lib(), stream_ptr(dev)
    gl = gl.to(torch.float32).contiguous() if gl is not None else None
    gr = gr.to(torch.float32).contiguous() if gr is not None else None
    ge = ge[0].to(dev, torch.float64).contiguous() if ge and ge[0] is not None else None
    if not wanted:
        return None, gl, gr, ge
    ray_grad = torch.empty((4, S * N), dtype=torch.float32, device=dev)
    ns = grad_slices(ray)
    from_grids = gl is not None or gr is not None or ge is None
    if from_grids:
        _lib.check(h.sdirt_forward_integral_grad_rays(
            ray.c_rays(), S, N, ps, ks, dptr(center), C.byref(dp) if dp is not None else None, _flags(rec.precision),
            dptr(gl), dptr(gr), None, ns, dptr(ray_grad), st))
    if ge is not None:
        _lib.check(h.sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dp), _flags(rec.precision), dptr(ge), None, ns,
                                          dptr(ray_grad), 1 if from_grids else 0, st))
    return ray_grad, gl, gr, ge


def points_bar(rec, ray_grad, smp):
    """p_bar [N, 3] float64 = dLoss/d(point_obj): sdirt_trace2sensor_grad_points on the record `rec` with the rays'
    upstream gradient ray_grad [4, M] fp32, summed over the slices in a fixed order."""
    ray = rec.ray
    S, N = ray.shape
    K, dev = rec.n_surfaces, ray.device
    if N == 0:
        return torch.zeros((0, 3), dtype=torch.float64, device=dev)
    h = _lib.lib()
    ns = grad_slices(ray)
    partial = torch.empty((N, ns, 3), dtype=torch.float64, device=dev)
    _lib.check(h.sdirt_trace2sensor_grad_points(
        rec.dev_lens.handle, (C.c_int32 * K)(*rec.trips), _flags(rec.precision), rec.d_sensor, dptr(rec.workspace),
        ray.c_rays().ra, dptr(ray_grad), S, N, dptr(smp.x2), dptr(smp.y2), smp.pupil_z, dptr(partial), ns, stream_ptr(dev)))
    return partial.sum(1)


def points_chain(points, p_bar, smp):
    """dLoss/d(points) [N, 3] float64 from p_bar = dLoss/d(point_obj) through point_obj = (x s W/2, y s H/2, z),
    s = -z tan(hfov) / r_last (optics.py:956-960, calc_scale_pinhole :1302-1306)."""
    p = points.detach().to(p_bar.device, torch.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    hw, hh, q = smp.sensor_w / 2, smp.sensor_h / 2, smp.tan_hfov / smp.r_last
    s = -z * q
    return torch.stack((p_bar[:, 0] * s * hw, p_bar[:, 1] * s * hh,
                        p_bar[:, 2] - (x * hw * p_bar[:, 0] + y * hh * p_bar[:, 1]) * q), -1)


class PointGradFunction(torch.autograd.Function):
    """An identity behind the raw grids (and the energy sums) of a psf call with point_grad=True.  Its backward takes
    ray_adjoint's dLoss/d(sensor-plane rays), walks the recorded trace back to the object points
    (sdirt_trace2sensor_grad_points) and applies the pinhole scale: the rays' share of dLoss/d(points).  The grids'
    gradients pass through unchanged."""

    @staticmethod
    def forward(ctx, points, lg, rg, rec, center, ps, ks, dp, smp, energy=None):
        ctx.rec, ctx.geom, ctx.dp, ctx.smp = rec, (float(ps), int(ks)), dp, smp
        ctx.meta = (points.dtype, points.device, tuple(points.shape))
        ctx.save_for_backward(center, points.detach())
        return _identity_outputs(ctx, lg, rg, energy)

    @staticmethod
    def backward(ctx, gl, gr, *ge):
        center, points = ctx.saved_tensors
        rec = ctx.rec
        wanted = ctx.needs_input_grad[0] and rec.ray.shape[1] > 0
        ray_grad, gl, gr, ge = ray_adjoint(rec, center, ctx.geom, ctx.dp, gl, gr, ge, wanted)
        g_points = None
        if wanted:
            dtype, device, shape = ctx.meta
            g_points = points_chain(points, points_bar(rec, ray_grad, ctx.smp), ctx.smp).to(device=device, dtype=dtype).reshape(shape)
        return (g_points, gl, gr, None, None, None, None, None, None) + ((ge,) if ctx.has_energy else ())


class ChiefCentreFunction(torch.autograd.Function):
    """points -> the chief-ray centres [N, 2] of a staged, recorded chief bundle (optics.py:889-904 without its
    no_grad): the values are `center` (sdirt_center_from_rays on the record's bundle).  The centre is
    c = -sum(o ra) / (sum ra + 1e-9), so with g_c = dLoss/dc the chief rays' sensor-plane adjoint is
    A.o.xy = -g_c ra / (sum ra + 1e-9), A.d = 0; it walks back like the primary bundle's."""

    @staticmethod
    def forward(ctx, points, center, rec, smp):
        ctx.rec, ctx.smp = rec, smp
        ctx.meta = (points.dtype, points.device, tuple(points.shape))
        ctx.save_for_backward(points.detach())
        return center.clone()

    @staticmethod
    def backward(ctx, gc):
        (points,) = ctx.saved_tensors
        rec = ctx.rec
        S, N = rec.ray.shape
        dev = rec.ray.device
        if gc is None or N == 0:
            return None, None, None, None
        ra = rec.ray.soa[6, :S * N].view(N, S).to(torch.float64)                   # point-major
        scale = -gc.to(dev, torch.float64).reshape(N, 2) / (ra.sum(1, keepdim=True) + 1e-9)
        ray_grad = torch.zeros((4, N, S), dtype=torch.float32, device=dev)
        ray_grad[0] = (scale[:, 0:1] * ra).to(torch.float32)
        ray_grad[1] = (scale[:, 1:2] * ra).to(torch.float32)
        dtype, device, shape = ctx.meta
        g = points_chain(points, points_bar(rec, ray_grad.view(4, N * S), ctx.smp), ctx.smp)
        return g.to(device=device, dtype=dtype).reshape(shape), None, None, None


class SurfaceGradFunction(torch.autograd.Function):
    """theta: surface parameters or None; eta: glass_eta(...) [K] or None (then the backward is the old entry's).
    energy: the [N, 3] sums of monte_carlo.dp_energy on the recorded bundle, or None.  With it the op has a third output,
    the sums, and dLoss/d(sums) reaches the rays as well (ray_adjoint: its terms in d.x, d.z) before the ONE walk."""

    @staticmethod
    def forward(ctx, theta, eta, lg, rg, rec, center, ps, ks, dp, energy=None):
        ctx.rec, ctx.geom, ctx.dp = rec, (float(ps), int(ks)), dp
        ctx.meta = [None if t is None else (t.dtype, t.device, tuple(t.shape)) for t in (theta, eta)]
        ctx.save_for_backward(center)
        return _identity_outputs(ctx, lg, rg, energy)

    @staticmethod
    def backward(ctx, gl, gr, *ge):
        (center,) = ctx.saved_tensors
        rec = ctx.rec
        ray = rec.ray
        M, K, dev = ray.shape[0] * ray.shape[1], rec.n_surfaces, ray.device
        h, st = _lib.lib(), stream_ptr(dev)
        ray_grad, gl, gr, ge = ray_adjoint(rec, center, ctx.geom, ctx.dp, gl, gr, ge)
        nwg = int(h.sdirt_trace2sensor_grad_workgroups(M, n_cus(dev)))
        theta_meta, eta_meta = ctx.meta
        with_eta = eta_meta is not None and ctx.needs_input_grad[1]
        entry = h.sdirt_trace2sensor_grad_eta if with_eta else h.sdirt_trace2sensor_grad
        partial = torch.empty((nwg, K, N_COLUMNS + (1 if with_eta else 0)), dtype=torch.float64, device=dev)
        _lib.check(entry(
            rec.dev_lens.handle, (C.c_int32 * K)(*rec.trips), _flags(rec.precision), rec.d_sensor, dptr(rec.workspace),
            ray.c_rays().ra, dptr(ray_grad), M, dptr(partial), nwg, st))
        total = partial.sum(0)                                               # the workgroups in a fixed order
        g_theta = g_eta = None
        if theta_meta is not None and ctx.needs_input_grad[0]:
            dtype, device, shape = theta_meta
            g_theta = total[:, :N_COLUMNS].to(device=device, dtype=dtype).reshape(shape)
        if with_eta:
            dtype, device, shape = eta_meta
            g_eta = total[:, N_COLUMNS].to(device=device, dtype=dtype).reshape(shape)
        # (the sums' own gradient goes on to EnergyFunction, which gives h, f, w theirs)
        return (g_theta, g_eta, gl, gr, None, None, None, None, None) + ((ge,) if ctx.has_energy else ())
