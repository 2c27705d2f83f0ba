"""A float64 torch restatement of a psf call as a function of its OBJECT POINTS: deeplens/optics.py:934-996 with the two
@torch.no_grad() decorators of sample_from_points (:459) and psf_center (:888) taken off and the pupil draws held fixed --
the yardstick of sdirt_trace2sensor_grad_points and of psf_lr(point_grad=True).

    point_obj = (x s W/2, y s H/2, z),  s = -z tan(hfov) / r_last          (optics.py:956-960, :1302-1306)
    o = point_obj repeated,  d = normalize(q_s - point_obj),  q_s = (x2[s], y2[s], pupil_z)      (:479-494, basics.py:245)

then trace_f64 (unchanged: every validity flag, Newton mask, t1 and clamp gate a forward decision) and psf_f64, or the
centre c = -sum(o ra) / (sum ra + 1e-9) (:903-904).  With checkpoints (the record's fp32 (o, d) on entry to every
surface) each surface is evaluated AT the kernel's own values while the derivative flows through the chain, so
autograd differentiates exactly the function the kernel differentiates, on the kernel's own rays.

Rays are point-major: ray (s, n) at n S + s.
"""
import torch

from splat_f64 import splat_f64  # noqa: F401  (the splat the restatement chains with, unchanged)
from trace_f64 import psf_f64, trace_f64

EPSILON = 1e-9


def object_points(points, tan_hfov, r_last, sensor_w, sensor_h):
    """optics.py:956-960 in the dtype of `points` [N, 3]."""
    scale = -points[:, 2] * tan_hfov / r_last
    return torch.stack((points[:, 0] * scale * sensor_w / 2, points[:, 1] * scale * sensor_h / 2, points[:, 2]), -1)


def chain(points, p_bar, tan_hfov, r_last, sensor_w, sensor_h, absolute=False):
    """dLoss/d(points) [N, 3] from p_bar = dLoss/d(point_obj) [N, 3], written out (the test of the library's chain
    compares it with autograd of object_points); absolute=True: every term's magnitude, for a p_bar of summed
    magnitudes -- the sum |terms| of the GPU tests' bars."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    hw, hh, q = sensor_w / 2, sensor_h / 2, tan_hfov / r_last
    s = -z * q
    if absolute:
        return torch.stack((p_bar[:, 0] * s.abs() * hw, p_bar[:, 1] * s.abs() * hh,
                            p_bar[:, 2] + (x.abs() * hw * p_bar[:, 0] + y.abs() * hh * p_bar[:, 1]) * q), -1)
    return torch.stack((p_bar[:, 0] * s * hw, p_bar[:, 1] * s * hh,
                        p_bar[:, 2] - (x * hw * p_bar[:, 0] + y * hh * p_bar[:, 1]) * q), -1)


def sample_rays(p, x2, y2, pupil_z, index=None):
    """(o, d) [M, 3] float64 of the point-major bundle from the points p [N, 3] to the pupil points (x2, y2 [S], pupil_z);
    p [N, S, 3]: every ray its own copy of its point (p.grad then holds the per-ray terms).  index: the rays kept
    (flat, n S + s), default all."""
    N, S = p.shape[0], x2.shape[0]
    q = torch.stack((x2.double(), y2.double(), torch.full_like(x2, float(pupil_z)).double()), -1)          # [S, 3]
    each = p if p.dim() == 3 else p.unsqueeze(1).expand(N, S, 3)
    o = each.reshape(-1, 3)
    v = (q.unsqueeze(0) - each).reshape(-1, 3)
    if index is not None:
        o, v = o[index], v[index]
    return o, v / v.norm(dim=-1, keepdim=True)


def sensor_rays(p, x2, y2, pupil_z, theta, table, trips, d_sensor, index=None, checkpoints=None):
    """Sensor-plane (o, d) of the kept rays as a function of the object points p [N, 3] float64."""
    o, d = sample_rays(p, x2, y2, pupil_z, index)
    return trace_f64(o, d, theta, table, trips, d_sensor, checkpoints)


def linear_form(p, x2, y2, pupil_z, theta, table, trips, d_sensor, ray_grad, index, checkpoints=None):
    """sum over the kept rays of ray_grad . (o.x, o.y, d.x, d.z) at the sensor: what the entry differentiates; ray_grad
    [4, len(index)] float64."""
    so, sd = sensor_rays(p, x2, y2, pupil_z, theta, table, trips, d_sensor, index, checkpoints)
    return (ray_grad[0] * so[:, 0] + ray_grad[1] * so[:, 1] + ray_grad[2] * sd[:, 0] + ray_grad[3] * sd[:, 2])


def centre(p, xc, yc, pupil_z, theta, table, trips, d_sensor, ra, checkpoints=None):
    """The chief-ray centres [N, 2] float64 (optics.py:903-904); ra [N S] the forward's weights (0 / 1).  Dead rays are
    replaced by the point's first live ray for the trace (they carry weight 0)."""
    N, S = p.shape[0], xc.shape[0]
    live = (ra != 0).reshape(N, S)
    first = live.float().argmax(1, keepdim=True) + torch.arange(N, device=p.device).unsqueeze(1) * S
    index = torch.where(live, torch.arange(N * S, device=p.device).reshape(N, S), first).reshape(-1)
    so, _ = sensor_rays(p, xc, yc, pupil_z, theta, table, trips, d_sensor, index,
                        None if checkpoints is None else checkpoints[:, :, index])
    w = ra.double().reshape(N, S, 1)
    c = (so.reshape(N, S, 3) * w).sum(1) / (w.sum(1) + EPSILON)
    return -c[:, :2]


def psf_of_points(p, x2, y2, pupil_z, theta, table, trips, d_sensor, center, ps, ks, dp, ra, checkpoints=None,
                  mask_dtype=torch.float32):
    """RAW (L, R) [N, ks, ks] float64 of the points p; ra [N S] the forward's weights; dead rays are replaced by the
    point's first live ray for the trace.  CPU tensors (splat_f64)."""
    N, S = p.shape[0], x2.shape[0]
    live = (ra != 0).reshape(N, S)
    first = live.float().argmax(1, keepdim=True) + torch.arange(N).unsqueeze(1) * S
    index = torch.where(live, torch.arange(N * S).reshape(N, S), first).reshape(-1)
    o, d = sample_rays(p, x2, y2, pupil_z, index)
    ck = None if checkpoints is None else checkpoints[:, :, index]
    return psf_f64(o, d, theta, table, trips, d_sensor, S, N, center, ps, ks, dp, checkpoints=ck, ra=ra.float(),
                   mask_dtype=mask_dtype)
