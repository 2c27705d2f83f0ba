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
from .monte_carlo import _flags

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


class SurfaceGradFunction(torch.autograd.Function):
    """theta: surface parameters or None; eta: glass_eta(...) [K] or None (then the backward is the old entry's).
    energy: the [N, 3] sums of monte_carlo.dp_energy on the recorded bundle, or None.  With it the op has a third output,
    the sums, and dLoss/d(sums) reaches the rays as well: sdirt_dp_energy_grad adds its terms in d.x, d.z to the splat's
    ray_grad (accumulate = 1) before the ONE walk -- or writes the buffer (accumulate = 0) when no gradient arrives from
    the grids."""

    @staticmethod
    def forward(ctx, theta, eta, lg, rg, rec, center, ps, ks, dp, energy=None):
        ctx.rec, ctx.geom, ctx.dp = rec, (float(ps), int(ks)), dp
        ctx.meta = [None if t is None else (t.dtype, t.device, tuple(t.shape)) for t in (theta, eta)]
        ctx.save_for_backward(center)
        ctx.has_energy = energy is not None
        if energy is None:
            return lg.clone(), rg.clone()
        ctx.set_materialize_grads(False)        # an output the loss does not use arrives as None, not as zeros
        return lg.clone(), rg.clone(), energy.clone()

    @staticmethod
    def backward(ctx, gl, gr, *ge):
        (center,) = ctx.saved_tensors
        rec, (ps, ks), dp = ctx.rec, ctx.geom, ctx.dp
        ray = rec.ray
        S, N = ray.shape
        M, K, dev = S * N, rec.n_surfaces, ray.device
        h, st = _lib.lib(), stream_ptr(dev)
        ncu = int(torch.cuda.get_device_properties(dev).multi_processor_count)
        gl = gl.to(torch.float32).contiguous() if gl is not None else None
        gr = gr.to(torch.float32).contiguous() if gr is not None else None
        ge = ge[0].to(dev, torch.float64).contiguous() if ge and ge[0] is not None else None
        ray_grad = torch.empty((4, M), dtype=torch.float32, device=dev)
        ns = int(h.sdirt_forward_integral_grad_slices(N, S, ncu))
        from_grids = gl is not None or gr is not None or ge is None
        if from_grids:
            _lib.check(h.sdirt_forward_integral_grad_rays(
                ray.c_rays(), S, N, ps, ks, dptr(center), C.byref(dp) if dp is not None else None, _flags(rec.precision),
                dptr(gl), dptr(gr), None, ns, dptr(ray_grad), st))
        if ge is not None:
            _lib.check(h.sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dp), _flags(rec.precision), dptr(ge), None, ns,
                                              dptr(ray_grad), 1 if from_grids else 0, st))
        nwg = int(h.sdirt_trace2sensor_grad_workgroups(M, ncu))
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
