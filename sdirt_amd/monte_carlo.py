"""Forward Monte-Carlo integral: sensor-plane rays -> dual-pixel PSF grids.

Same call signatures as deeplens/monte_carlo.py (forward_integral :9,
assign_points_to_pixels_small_r :135, _big_r :242); the work is one HIP kernel
(sdirt_forward_integral): window test, closed-form left/right sub-pixel areas
and the 4-tap bilinear scatter-add.  dp_energy (sdirt_dp_energy) sums the same
sub-pixel areas over ALL rays of a point: the energy the window and the
normalisations of the PSF path discard.
"""
import ctypes as C

import torch

from . import _lib
from .basics import Ray, dptr, stream_ptr


def _dp(param_list):
    if param_list is None:
        return None, "l"
    h, f, w, r, direct = param_list
    return _lib.DpParams(float(h), float(f), float(w), float(r)), direct


def n_cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def grad_slices(ray):
    """n_slices of every launch that cuts the spp axis of the bundle `ray` [S, N] as the splat's backward does
    (sdirt_forward_integral_grad_slices on the bundle's device)."""
    S, N = ray.shape
    return int(_lib.lib().sdirt_forward_integral_grad_slices(N, S, n_cus(ray.device)))


def _requires_grad(*vals):
    """Whether autograd is recording and one of `vals` (tensors, Python numbers, None) requires a gradient."""
    return torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in vals)


class SplatFunction(torch.autograd.Function):
    """The splat stage as an autograd op: (h, f, w, centres) -> RAW (l_grid, r_grid) [N, ks, ks] of
    sdirt_forward_integral, differentiable in h, f, w (0-d tensors; Python numbers get no gradient) and in the
    centres [N, 2] (pointc_ref).  The rays, r and the precision are constants, as in the reference (its rays are
    sampled under no_grad, r is re-wrapped by torch.tensor(r) at monte_carlo.py:167, :274).  The backward is one
    kernel, sdirt_forward_integral_grad, on the same rays, centres and parameters: the forward's window, taps and
    clamp decisions, float64 sums, no atomics.

    d_sensor (a 0-d tensor, or None): the sensor position the rays were propagated to.  When it requires a gradient the
    backward is sdirt_forward_integral_grad_focus instead -- the same five sums and a sixth, the rays' own share
    sum(g_x d.x / d.z + g_y d.y / d.z) -- and center_slope ([N, 2] float64 d(centre)/d(d_sensor) of the chief-ray
    centres, sdirt_chief_center_slope; None for centres that do not move with the sensor) adds the centres' share:
    dLoss/ds = sum_n (ds_n + dcx_n slope_n,x + dcy_n slope_n,y).  The value of d_sensor is not used here."""

    @staticmethod
    def forward(ctx, h, f, w, center, ray, ps, ks, r, have_dp, precision, d_sensor=None, center_slope=None):
        S, N = ray.shape
        dev = ray.device
        center = center.detach().to(dev, torch.float32).reshape(N, 2).contiguous()
        dp = _lib.DpParams(float(h), float(f), float(w), float(r)) if have_dp else None
        lg = torch.empty((N, ks, ks), dtype=torch.float32, device=dev)
        rg = torch.empty_like(lg)
        _lib.check(_lib.lib().sdirt_forward_integral(
            ray.c_rays(), S, N, float(ps), int(ks), dptr(center), C.byref(dp) if dp is not None else None,
            _flags(precision), dptr(lg), dptr(rg), stream_ptr(dev)))
        ctx.ray, ctx.dp, ctx.geom, ctx.precision = ray, dp, (S, N, float(ps), int(ks)), precision
        ctx.meta = [(v.dtype, v.device) if torch.is_tensor(v) else None for v in (h, f, w, d_sensor)]
        ctx.center_slope = center_slope
        ctx.save_for_backward(center)
        return lg, rg

    @staticmethod
    def backward(ctx, gl, gr):
        (center,) = ctx.saved_tensors
        S, N, ps, ks = ctx.geom
        dev = center.device
        ns = grad_slices(ctx.ray)
        focus = ctx.needs_input_grad[10]
        partial = torch.empty((N, ns, 6 if focus else 5), dtype=torch.float64, device=dev)
        gl = gl.to(torch.float32).contiguous() if gl is not None else None
        gr = gr.to(torch.float32).contiguous() if gr is not None else None
        dp = ctx.dp
        entry = _lib.lib().sdirt_forward_integral_grad_focus if focus else _lib.lib().sdirt_forward_integral_grad
        _lib.check(entry(
            ctx.ray.c_rays(), S, N, ps, ks, dptr(center), C.byref(dp) if dp is not None else None,
            _flags(ctx.precision), dptr(gl), dptr(gr), dptr(partial), ns, stream_ptr(dev)))
        tot = partial.sum(1)                                   # [N, 5 or 6] float64: the slices in a fixed order
        theta = tot[:, :3].sum(0)
        grads = [theta[i].to(device=ctx.meta[i][1], dtype=ctx.meta[i][0]) if ctx.needs_input_grad[i] else None
                 for i in range(3)]
        gc = tot[:, 3:5].to(torch.float32) if ctx.needs_input_grad[3] else None
        gs = None
        if focus:
            per_point = tot[:, 5]
            if ctx.center_slope is not None:                   # the chief-ray centres move with the sensor
                per_point = per_point + (tot[:, 3:5] * ctx.center_slope.to(dev, torch.float64)).sum(1)
            gs = per_point.sum(0).to(device=ctx.meta[3][1], dtype=ctx.meta[3][0])
        return (*grads, gc, None, None, None, None, None, None, gs, None)


def _as_scalar(v):
    """A DP parameter as SplatFunction takes it: a tensor that requires grad stays itself (autograd casts the
    gradient back to its dtype and device), anything else becomes a plain number."""
    return v.reshape(()) if torch.is_tensor(v) and v.requires_grad else float(v)


def splat_autograd(ray, ps, ks, center, param_list, precision="lean", d_sensor=None, center_slope=None):
    """RAW (l_grid, r_grid) through SplatFunction: param_list = (h, f, w, r, direct) or None (the reference's
    defaults, R all zero); r and direct get no gradient.  The grids are NOT swapped for direct != 'l'.
    d_sensor / center_slope: the sensor position as a 0-d tensor that requires a gradient and the slope of the
    chief-ray centres in it (SplatFunction); None: the sensor position is a constant."""
    have_dp = param_list is not None
    h, f, w, r = (param_list[:4] if have_dp else (0.78, 1.44, 0.3, 0.5))
    h, f, w = (_as_scalar(v) for v in (h, f, w))
    if d_sensor is not None:
        d_sensor = d_sensor.reshape(())
    return SplatFunction.apply(h, f, w, center, ray, ps, ks, float(r), have_dp, precision, d_sensor, center_slope)


class EnergyFunction(torch.autograd.Function):
    """The energy of every point as an autograd op: (h, f, w) -> [N, 3] float64 sums over ALL spp rays of the
    sensor-plane bundle (sum ra s_l, sum ra s_r, sum ra), s_l / s_r the splat's own sub-pixel areas at
    x_tan = -d.x / d.z (sdirt_dp_energy).  Differentiable in h, f, w exactly as SplatFunction is (0-d tensors; Python
    numbers get no gradient); the rays, r and the precision are constants, and column 2 has no gradient to give.
    d_sensor (a 0-d tensor or None) gets a gradient of exactly 0: the propagation to the sensor plane changes neither a
    ray's direction nor its weight."""

    @staticmethod
    def forward(ctx, h, f, w, ray, r, precision, d_sensor=None):
        S, N = ray.shape
        dev = ray.device
        dp = _lib.DpParams(float(h), float(f), float(w), float(r))
        ctx.ray, ctx.dp, ctx.precision = ray, dp, precision
        ctx.meta = [(v.dtype, v.device) if torch.is_tensor(v) else None for v in (h, f, w, d_sensor)]
        if N == 0:
            return torch.zeros((0, 3), dtype=torch.float64, device=dev)
        ns = grad_slices(ray)
        partial = torch.empty((N, ns, 3), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().sdirt_dp_energy(ray.c_rays(), S, N, C.byref(dp), _flags(precision), dptr(partial), ns,
                                              stream_ptr(dev)))
        return partial.sum(1)                                  # the slices in a fixed order

    @staticmethod
    def backward(ctx, ge):
        ray = ctx.ray
        S, N = ray.shape
        dev = ray.device
        theta = torch.zeros(3, dtype=torch.float64, device=dev)
        if N > 0 and any(ctx.needs_input_grad[:3]):
            ns = grad_slices(ray)
            ge = ge.to(dev, torch.float64).contiguous()
            partial = torch.empty((N, ns, 3), dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(ctx.dp), _flags(ctx.precision), dptr(ge),
                                                       dptr(partial), ns, None, 0, stream_ptr(dev)))
            theta = partial.sum(1).sum(0)
        grads = [theta[i].to(device=ctx.meta[i][1], dtype=ctx.meta[i][0]) if ctx.needs_input_grad[i] else None
                 for i in range(3)]
        gs = torch.zeros((), dtype=ctx.meta[3][0], device=ctx.meta[3][1]) if ctx.needs_input_grad[6] else None
        return (*grads, None, None, None, gs)


def dp_energy(ray, param_list, precision="lean", d_sensor=None):
    """[N, 3] float64: per point of the [spp, N] sensor-plane bundle `ray` the sums over ALL its rays, inside the PSF
    window or not, of (ra d_l(x_tan), ra d_r(x_tan), ra) -- d_l, d_r the closed-form sub-pixel areas of
    assign_points_to_pixels_small_r / _big_r (monte_carlo.py:135-240, 242-372) the splat weighs a ray with, in the
    fp32 the splat computes them in.  Divided by spp: the left and right energy of the point and the share of its rays
    that arrive -- the vignetting and the dual-pixel shading forward_integral's window and the PSF normalisations
    discard.  param_list = (h, f, w, r[, direct]); differentiable in tensor h, f, w (EnergyFunction), r and the rays
    are constants.  d_sensor: a 0-d tensor that gets a gradient of exactly 0."""
    if len(ray.shape) != 2:
        raise ValueError("ray must have shape [spp, N]")
    if param_list is None:
        raise ValueError("dp_energy needs the dual-pixel parameters (h, f, w, r)")
    h, f, w = (_as_scalar(v) for v in param_list[:3])
    if d_sensor is not None:
        d_sensor = d_sensor.reshape(())
    return EnergyFunction.apply(h, f, w, ray, float(param_list[3]), precision, d_sensor)


def _flags(precision):
    if precision not in ("lean", "ieee"):
        raise ValueError("precision must be 'lean' or 'ieee'")
    return _lib.PSF_STRICT_IEEE if precision == "ieee" else 0


def forward_integral_lr(ray, ps, ks, pointc_ref=None, param_list=None, precision="lean"):
    """RAW (l_grid, r_grid), each [N, ks, ks]; r_grid is all-zero when
    param_list is None exactly as in monte_carlo.py:230-235.  precision='ieee': the reference's literal
    sequence for the sub-pixel areas (arccos, sin) and the compiler's full-range divisions instead of the
    fused segment-area polynomial (SDIRT_PSF_STRICT_IEEE).  Differentiable in param_list's h, f, w and in
    pointc_ref when one of them requires a gradient (SplatFunction); otherwise the grids carry no grad_fn.
    (The RMS centre of pointc_ref=None depends on the rays only, and the rays carry no gradient.)"""
    if len(ray.shape) != 2:
        raise ValueError("ray must have shape [spp, N]")
    S, N = ray.shape
    dev = ray.device
    grad = _requires_grad(pointc_ref, *(param_list[:3] if param_list is not None else ()))
    if pointc_ref is None:
        # RMS centre, monte_carlo.py:28-31
        center = torch.empty((N, 2), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().sdirt_center_from_rays(ray.c_rays(), S, N, dptr(center), None,
                                                     stream_ptr(dev)))
    elif grad:
        center = pointc_ref.to(dev, torch.float32).reshape(N, 2)
    else:
        center = pointc_ref.to(dev, torch.float32).reshape(N, 2).contiguous()
    if grad:
        # h, f, w or pointc_ref require a gradient: the same forward kernel behind SplatFunction
        return splat_autograd(ray, ps, ks, center, param_list, precision)
    dp, _ = _dp(param_list)
    lg = torch.empty((N, ks, ks), dtype=torch.float32, device=dev)
    rg = torch.empty_like(lg)
    _lib.check(_lib.lib().sdirt_forward_integral(
        ray.c_rays(), S, N, float(ps), int(ks), dptr(center),
        C.byref(dp) if dp is not None else None, _flags(precision), dptr(lg), dptr(rg), stream_ptr(dev)))
    return lg, rg


def forward_integral(ray, ps, ks, pointc_ref=None, interpolate=False, param_list=None, precision="lean"):
    """monte_carlo.py:9-68 -> [N, ks, ks]: the left grid, or the right one when
    param_list[4] != 'l' (the reference returns `psf_l` of a swapped pair, :64,237-240)."""
    lg, rg = forward_integral_lr(ray, ps, ks, pointc_ref, param_list, precision)
    _, direct = _dp(param_list)
    return lg if direct == "l" else rg


def _assign(points, ks, x_range, ra, x_tan, param_list, big, precision="lean"):
    if param_list is None:
        r = 0.5
    else:
        r = param_list[3]
    assert (r >= 0.5) if big else (r <= 0.5)
    dev = points.device
    if dev.type != "cuda":
        raise _lib.SdirtError("sdirt_amd splats on the GPU only (no CPU fallback)")
    S = points.shape[0]
    ps = (x_range[1] - x_range[0]) / (ks - 1)
    # forward_integral negates o and divides -d_x by d_z: feed o = -points,
    # d = (-x_tan, 0, 1) so that the kernel sees exactly `points` and `x_tan`.
    ray = Ray.empty((S, 1), device=dev)
    pts = points.to(torch.float32).reshape(S, 2)
    ray.soa[0, :S] = -pts[:, 0]
    ray.soa[1, :S] = -pts[:, 1]
    ray.soa[2, :S] = 0.0
    ray.soa[3, :S] = -x_tan.to(torch.float32).reshape(S)
    ray.soa[4, :S] = 0.0
    ray.soa[5, :S] = 1.0
    ray.soa[6, :S] = ra.to(torch.float32).reshape(S)
    center = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    if big and param_list is None:
        param_list = [0.78, 1.44, 0.3, 0.5, "l"]
    lg, rg = forward_integral_lr(ray, ps, ks, center, param_list, precision)
    lg, rg = lg[0], rg[0]
    direct = "l" if param_list is None else param_list[4]
    return (lg, rg) if direct == "l" else (rg, lg)


def assign_points_to_pixels_small_r(points, ks, x_range, y_range, ra, interpolate=True,
                                    coherent=False, phase=None, d=None, obliq=None, wvln=0.589,
                                    x_tan=None, param_list=None, precision="lean"):
    """monte_carlo.py:135-240 for one point source: points [spp,2] inside the
    PSF window, ra [spp], x_tan [spp] -> (l_grid, r_grid) [ks,ks]."""
    return _assign(points, ks, x_range, ra, x_tan, param_list, big=False, precision=precision)


def assign_points_to_pixels_big_r(points, ks, x_range, y_range, ra, interpolate=True,
                                  coherent=False, phase=None, d=None, obliq=None, wvln=0.589,
                                  x_tan=None, param_list=None):
    """monte_carlo.py:242-372 (microlens radius r >= 0.5)."""
    return _assign(points, ks, x_range, ra, x_tan, param_list, big=True)
