"""A float64 torch restatement of a dual-pixel PSF as a function of the sensor position s (the focus setting),
differentiable by torch's own autograd: the specification of DESIGN.md 7h and the yardstick of
sdirt_forward_integral_grad_focus and sdirt_chief_center_slope.

A ray that leaves the last surface at o' with direction d meets the sensor plane z = s at
    o(s) = o' + d (s - o'.z) / d.z,        d o.xy / ds = d.xy / d.z.
Rays are given where the forward put them: their sensor-plane points at s0 (ox, oy) and their directions (dx, dy, dz),
[S, N], as the float32 arrays the kernels read or as float64 arrays of a reference run; sensor_points moves them to s.
x_tan = -d.x / d.z and the weights ra do not depend on s.  The window test, the taps and the clamp decisions are
splat_f64's: taken on the values, they carry no gradient.

The centre: with center=True the chief-ray centroid c(s) = -sum(ra o(s).xy) / (sum(ra) + 1e-9) over the green chief
rays (chief_centre) -- it moves with the sensor at first order, and that motion is part of the derivative (the
reference computes it under no_grad; `centre_in_graph=False` restates that).  With center=False the pinhole centres,
which do not depend on s.  The splat shifts by -o - c, so o and c enter alike.

s may be a 0-d leaf or an [S, N] tensor of per-ray leaves (their gradients are the per-ray terms: the sum of their
magnitudes is the scale the kernel's error is measured in); for the chief rays an [Sc, N] tensor likewise.
"""
import torch

from splat_f64 import max_normalise, splat_f64


def slopes(dx, dy, dz):
    """d(o.xy)/ds per ray, float64: (d.x / d.z, d.y / d.z)."""
    z = dz.double()
    return dx.double() / z, dy.double() / z


def sensor_points(ox, oy, dx, dy, dz, s, s0):
    """(o.x, o.y)(s), float64 [S, N], of rays that are at (ox, oy) when the sensor sits at s0."""
    mx, my = slopes(dx, dy, dz)
    return ox.double() + mx * (s - s0), oy.double() + my * (s - s0)


def chief_centre(cox, coy, cdx, cdy, cdz, cra, s, s0):
    """c(s) [N, 2], float64: minus the ra-weighted mean of the chief rays' sensor-plane points (optics.py:903-904).
    A ray without weight contributes nothing, whatever direction the trace left it with."""
    live = cra != 0
    one = torch.ones_like(cdz)
    x, y = sensor_points(cox, coy, torch.where(live, cdx, 0 * one), torch.where(live, cdy, 0 * one),
                         torch.where(live, cdz, one), s, s0)
    ra = cra.double()
    den = ra.sum(0) + 1e-9
    return torch.stack((-(ra * x).sum(0) / den, -(ra * y).sum(0) / den), -1)


def chief_slope_terms(cdx, cdy, cdz, cra):
    """The per-ray terms ra d.xy / d.z of dc/ds = -sum(terms) / (sum(ra) + 1e-9): float64 [Sc, N, 2], 0 for a ray
    without weight.  The same float64 operations, one by one, as k_chief_center<SLOPE>'s."""
    live = cra != 0
    z = torch.where(live, cdz, torch.ones_like(cdz)).double()
    ra = cra.double()
    tx = torch.where(live, ra * (cdx.double() / z), torch.zeros_like(z))
    ty = torch.where(live, ra * (cdy.double() / z), torch.zeros_like(z))
    return torch.stack((tx, ty), -1)


def raw_psf(rays, s, s0, centre, ps, ks, h, f, w, r, mask_dtype=torch.float32):
    """RAW (L, R) [N, ks, ks] float64 with the sensor at s.  rays = (ox, oy, dx, dy, dz, ra) [S, N] at s0; centre
    [N, 2] (or per-ray [S, N, 2]): chief_centre(..., s, s0) for the centre in the graph, a constant otherwise.
    The window is tested on the points' values at s (at s = s0: the forward's own)."""
    ox, oy, dx, dy, dz, ra = rays
    x, y = sensor_points(ox, oy, dx, dy, dz, s, s0)
    return splat_f64(x, y, dx, dz, ra, centre, ps, ks, h, f, w, r, mask_dtype=mask_dtype)


def psf_lr(rays, chief, s, s0, ps, ks, dp, pinhole=None, centre_in_graph=True, mask_dtype=torch.float32,
           chief_s=None, centre_value=None):
    """The max-normalised (L, R) [N, ks, ks] of psf_lr(dp=dp) with the sensor at s.
    chief = (cox, coy, cdx, cdy, cdz, cra) [Sc, N] at s0 (center=True) or None with pinhole = the centres [N, 2]
    (center=False).  centre_in_graph=False: the centre's value at s, detached.  chief_s: another leaf (or per-ray
    leaves) for the centre's share of the gradient; default s.  centre_value [N, 2]: the centre's VALUE (a kernel's own
    fp32 centres), its derivative still chief_centre's."""
    if chief is not None:
        c = chief_centre(*chief, s if chief_s is None else chief_s, s0)
        if centre_value is not None:
            c = torch.as_tensor(centre_value).double() + (c - c.detach())
        if not centre_in_graph:
            c = c.detach()
    else:
        c = torch.as_tensor(pinhole).double()
    h, f, w, r = dp
    L, R = raw_psf(rays, s, s0, c, ps, ks, h, f, w, float(r), mask_dtype=mask_dtype)
    return max_normalise(L), max_normalise(R)


def psf(rays, chief, s, s0, ps, ks, dp, direct="l", **kw):
    """The max-normalised PSF [N, ks, ks] of psf_diff(param_list=[*dp, direct]) with the sensor at s (psf_lr's
    arguments)."""
    L, R = psf_lr(rays, chief, s, s0, ps, ks, dp, **kw)
    return L if direct == "l" else R
