"""The backward pass of the staged trace as an autograd op: surface parameters theta [K, 3 + MAX_AI] (columns d, c, k,
ai2, ai4, ...) get the gradient the reference's graph gives them (deeplens/surfaces.py:523-679 under autograd).

The forward of a psf call with `surface_params=` is the staged chain with a RECORDING trace (sdirt_trace2sensor_record:
every ray's (o, d) on entry to each surface); the raw grids come from monte_carlo.SplatFunction as in every other
differentiable call.  SurfaceGradFunction sits behind those grids as an identity: its backward receives dLoss/d(raw
grids), turns it into dLoss/d(sensor-plane rays) (sdirt_forward_integral_grad_rays) and walks the recorded trace
backwards (sdirt_trace2sensor_grad); the grids' gradients pass through unchanged to SplatFunction, so h, f, w and the
pinhole centres get theirs in the same backward.
"""
import ctypes as C

import torch

from . import _lib
from .basics import dptr, stream_ptr
from .monte_carlo import _flags

N_COLUMNS = 3 + _lib.MAX_AI


class TraceRecord:
    """What the backward needs of one recorded trace: the device lens (kept alive), the trip table and math policy of the
    recording launch, the sensor plane, the checkpoints and the sensor-plane bundle."""

    def __init__(self, dev_lens, trips, precision, d_sensor, workspace, ray, n_surfaces):
        self.dev_lens, self.trips, self.precision, self.d_sensor = dev_lens, [int(t) for t in trips], precision, float(d_sensor)
        self.workspace, self.ray, self.n_surfaces = workspace, ray, int(n_surfaces)
        self.center = None          # the [N, 2] centres the splat used (set by the psf call)


class SurfaceGradFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, lg, rg, rec, center, ps, ks, dp):
        ctx.rec, ctx.geom, ctx.dp = rec, (float(ps), int(ks)), dp
        ctx.meta = (theta.dtype, theta.device, tuple(theta.shape))
        ctx.save_for_backward(center)
        return lg.clone(), rg.clone()

    @staticmethod
    def backward(ctx, gl, gr):
        (center,) = ctx.saved_tensors
        rec, (ps, ks), dp = ctx.rec, ctx.geom, ctx.dp
        ray = rec.ray
        S, N = ray.shape
        M, K, dev = S * N, rec.n_surfaces, ray.device
        h, st = _lib.lib(), stream_ptr(dev)
        ncu = int(torch.cuda.get_device_properties(dev).multi_processor_count)
        gl = gl.to(torch.float32).contiguous() if gl is not None else None
        gr = gr.to(torch.float32).contiguous() if gr is not None else None
        ray_grad = torch.empty((4, M), dtype=torch.float32, device=dev)
        ns = int(h.sdirt_forward_integral_grad_slices(N, S, ncu))
        _lib.check(h.sdirt_forward_integral_grad_rays(
            ray.c_rays(), S, N, ps, ks, dptr(center), C.byref(dp) if dp is not None else None, _flags(rec.precision),
            dptr(gl), dptr(gr), None, ns, dptr(ray_grad), st))
        nwg = int(h.sdirt_trace2sensor_grad_workgroups(M, ncu))
        partial = torch.empty((nwg, K, N_COLUMNS), dtype=torch.float64, device=dev)
        _lib.check(h.sdirt_trace2sensor_grad(
            rec.dev_lens.handle, (C.c_int32 * K)(*rec.trips), _flags(rec.precision), rec.d_sensor, dptr(rec.workspace),
            ray.c_rays().ra, dptr(ray_grad), M, dptr(partial), nwg, st))
        dtype, device, shape = ctx.meta
        g = partial.sum(0).to(device=device, dtype=dtype).reshape(shape)     # the workgroups in a fixed order
        return g, gl, gr, None, None, None, None, None
