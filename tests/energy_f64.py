"""A float64 torch restatement of the energy of a point (sdirt_dp_energy): the sums over ALL its rays, inside the PSF
window or not, of ra * area_l, ra * area_r and ra, with the sub-pixel areas of tests/splat_f64.py (sub_pixel_areas, which
tests/test_dp_grad_cpu.py holds against the reference's own autograd) at t = -dx / dz in float64.

Rays are given as the float32 arrays the kernels read (dx, dz, ra: [S, N]).  A ray with ra = 0 contributes exactly 0
whatever its direction holds (a traced bundle's dead rays may carry anything)."""
import torch

from splat_f64 import sub_pixel_areas


def x_tan_f64(dx, dz, ra):
    """t = -dx / dz in float64 [S, N]; 0 for a ray without weight."""
    live = ra != 0
    one = torch.ones_like(dz, dtype=torch.float64)
    return torch.where(live, -dx.double() / torch.where(live, dz.double(), one), torch.zeros_like(one))


def energy_terms_f64(dx, dz, ra, h, f, w, r):
    """Per ray (ra * area_l, ra * area_r, ra), each float64 [S, N]."""
    t = x_tan_f64(dx, dz, ra)
    sl, sr = sub_pixel_areas(t, h, f, w, r)
    wgt = ra.double()
    return wgt * sl, wgt * sr, wgt + 0 * t


def energy_f64(dx, dz, ra, h, f, w, r):
    """[N, 3] float64: (sum ra area_l, sum ra area_r, sum ra) over the spp axis."""
    return torch.stack([v.sum(0) for v in energy_terms_f64(dx, dz, ra, h, f, w, r)], -1)


def energy_scale_f64(dx, dz, ra, h, f, w, r):
    """[N, 3] float64: the sums of the magnitudes of the terms of energy_f64, the scale of its rounding."""
    return torch.stack([v.abs().sum(0) for v in energy_terms_f64(dx, dz, ra, h, f, w, r)], -1)


def energy_grad_f64(dx, dz, ra, h, f, w, r, grad_e):
    """The backward pass by per-ray leaves: for the loss sum(grad_e[:, :2] * energy_f64[:, :2]) (grad_e [N, 3] float64,
    column 2 unused: ra carries no gradient) ->
      theta [3], theta_scale [3]: the sums over all rays of the per-ray gradients in (h, f, w) and of their magnitudes;
      per_point [N, 3], per_point_scale [N, 3]: the same per point;
      g_dx, g_dz [S, N]: every ray's gradient in its direction components, through t = -dx / dz."""
    S, N = dx.shape
    hv, fv, wv = (torch.full((S, N), float(v), dtype=torch.float64, requires_grad=True) for v in (h, f, w))
    live = ra != 0
    dxv = torch.where(live, dx.double(), torch.zeros((), dtype=torch.float64)).requires_grad_(True)
    dzv = torch.where(live, dz.double(), torch.ones((), dtype=torch.float64)).requires_grad_(True)
    t = -dxv / dzv
    sl, sr = sub_pixel_areas(t, hv, fv, wv, r)
    wgt = ra.double()
    g = grad_e.double()
    ((wgt * sl).sum(0) * g[:, 0] + (wgt * sr).sum(0) * g[:, 1]).sum().backward()
    zero = torch.zeros((S, N), dtype=torch.float64)
    gs = [v.grad if v.grad is not None else zero for v in (hv, fv, wv)]
    per_point = torch.stack([v.sum(0) for v in gs], -1)
    per_point_scale = torch.stack([v.abs().sum(0) for v in gs], -1)
    g_dx = dxv.grad if dxv.grad is not None else zero
    g_dz = dzv.grad if dzv.grad is not None else zero
    return dict(theta=per_point.sum(0), theta_scale=per_point_scale.sum(0), per_point=per_point,
                per_point_scale=per_point_scale, g_dx=g_dx * live, g_dz=g_dz * live)
