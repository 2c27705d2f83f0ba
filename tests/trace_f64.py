"""A float64 torch restatement of the forward trace to the sensor (deeplens/optics.py:638-664 with Aspheric.ray_reaction,
_newtons_method, _normal, _refract of surfaces.py:391-679 and Ray.propagate_to), differentiable by torch's own autograd in
the surface parameters theta [K, 3 + MAX_AI] (columns d, c, k, ai2, ai4, ...): the yardstick of sdirt_trace2sensor_grad.

The sag and its r2-derivative are the reference's literal expressions (_g, _dgd).  The no-grad Newton loop runs the
trips of a given trip table; t1 is detached and the regain step t = t0 + t1 - clamp(ft / (dfdt + 1e-9), +-5) carries the
graph, as surfaces.py:563-578.  Validity carries no gradient: the caller passes the rays that are alive at the sensor
(the forward's own decision) and only those are traced, so every validity flag is 1; the `_valid` mask of the regain step
is evaluated on the values at hand.

checkpoints: the fp32 (o, d) a recording kernel stored on entry to every surface and before the final propagation
([K + 1, 6, M]).  When given, every surface is evaluated AT the checkpoint's values while the derivative by theta still
flows through the chain (value + (x - x.detach())): the restatement then differentiates exactly the function the kernel
differentiates, on the kernel's own rays.

theta may be [K, C] or per-ray leaves [M, K, C] (every ray its own copy: theta.grad then holds the per-ray terms).
Chained with splat_f64 (psf_f64, CPU tensors) it restates a raw PSF.  trace_f64 runs on the device of `o`.
"""
import torch

from splat_f64 import splat_f64

EPS = 1e-9
STEP_BOUND = 5.0
PLANE, SPHERE, ASPHERE = 0, 1, 2
CONIC = {"rf50mm": {8: -1.3, 9: 0.4}, "rf35mm": {10: 0.5}}      # conic constants for the aspheres of the test lenses


def lens_table(lens, wvln):
    """What the restatement needs of a sdirt_amd Lensgroup besides theta: per surface (kind, ai_degree, semi-aperture r,
    eta = n1 / n2 at `wvln`, and the values of c and k that pick the code's branches)."""
    wv = wvln if wvln < 10 else wvln * 1e-3
    return [(s.kind, s.ai_degree if s.kind == ASPHERE else 0, float(s.r), float(s.mat1.ior(wv)) / float(s.mat2.ior(wv)),
             float(s.c), float(s.k)) for s in lens.surfaces]


def with_conic(lens, conic):
    """`lens` with the conic constants {surface: k} written into its records (None: as it is).  A k != 0 makes k a
    parameter of an asphere, which no shipped lens has; set_surface_parameters cannot do it, since the column is not
    owned before the write."""
    for i, v in (conic or {}).items():
        lens.surfaces[i].k = type(lens.surfaces[i].k)(v)
    return lens.set_surface_parameters(lens.surface_parameters()) if conic else lens


def _g(r2, c, k, ai):
    z = r2 * c / (1 + torch.sqrt(1 - (1 + k) * r2 * c ** 2))
    for i, a in enumerate(ai):
        z = z + a * r2 ** (i + 1)
    return z


def _dgd(r2, c, k, ai):
    sf = torch.sqrt(1 - (1 + k) * r2 * c ** 2)
    z = (1 + sf + (1 + k) * r2 * c ** 2 / 2 / sf) * c / (1 + sf) ** 2
    for i, a in enumerate(ai):
        z = z + (i + 1) * a * r2 ** i
    return z


def _refract(d, n, eta):
    cosi = (d * n).sum(-1, keepdim=True)
    sr = torch.sqrt(1 - eta ** 2 * (1 - cosi ** 2))
    return sr * n + eta * (d - cosi * n)


def _residual(o, d, t, valid, D, c, k, ai):
    p = o + d * t.unsqueeze(-1)
    x, y = p[:, 0] * valid, p[:, 1] * valid
    r2 = x ** 2 + y ** 2
    ft = _g(r2, c, k, ai) + D - p[:, 2]
    dr2dt = 2 * ((d[:, 0] ** 2 + d[:, 1] ** 2) * t + (d[:, 0] * o[:, 0] + d[:, 1] * o[:, 1]))
    return ft, _dgd(r2, c, k, ai) * dr2dt - d[:, 2]


def surface_f64(o, d, row, kind, deg, r_ap, eta, c0, k0, trips):
    """Aspheric.ray_reaction for rays that stay valid: (o, d) [M, 3] float64 -> (o', d').  row[j]: column j of this
    surface's parameters (scalars, or [M] per-ray copies); c0, k0: the values of c and k, for the branches."""
    D, c, k, ai = row[0], row[1], row[2], [row[3 + i] for i in range(deg)]
    if kind == PLANE:
        t = (D - o[:, 2]) / d[:, 2]
        o = o + t.unsqueeze(-1) * d
        if eta != 1:
            n = torch.zeros_like(o)
            n[:, 2] = 1.0                                  # -normalize((0, 0, -1)): forward
            d = _refract(d, n, eta)
        return o, d
    t0 = (D - o[:, 2]) / d[:, 2]
    with torch.no_grad():
        t = t0.clone()
        for _ in range(int(trips)):
            p = o + d * t.unsqueeze(-1)
            rr = p[:, 0] ** 2 + p[:, 1] ** 2
            loose = (rr < (1 - EPS) / c ** 2 / (1 + k)) if k0 > -1 else (rr > 0)
            ft, dfdt = _residual(o, d, t, loose.double(), D, c, k, ai)
            t = t - torch.clamp(ft / (dfdt + EPS), -STEP_BOUND, STEP_BOUND)
        t1 = t - t0
    t = t0 + t1
    with torch.no_grad():
        p = o + d * t.unsqueeze(-1)
        rr = p[:, 0] ** 2 + p[:, 1] ** 2
        valid = rr < r_ap ** 2
        if k0 > -1:
            valid = valid & (rr < (1 - EPS) / c ** 2 / (1 + k))
    ft, dfdt = _residual(o, d, t, valid.double(), D, c, k, ai)
    t = t - torch.clamp(ft / (dfdt + EPS), -STEP_BOUND, STEP_BOUND)
    o = o + t.unsqueeze(-1) * d
    x, y, z = o[:, 0], o[:, 1], o[:, 2]
    if kind == SPHERE:
        sg = 2.0 if c0 > 0 else -2.0
        n = torch.stack((sg * x, sg * y, sg * z - sg * (D + 1 / c)), -1)
    else:
        h = _dgd(x ** 2 + y ** 2, c, k, ai)
        n = torch.stack((h * 2 * x, h * 2 * y, -torch.ones_like(x)), -1)
    n = -torch.nn.functional.normalize(n, p=2, dim=-1)
    return o, _refract(d, n, eta)


def _at(value, x):
    """`value` with the derivative of x."""
    return value + (x - x.detach())


def trace_f64(o, d, theta, table, trips, d_sensor, checkpoints=None):
    """Sensor-plane (o, d) [M, 3] float64 of the rays (o, d) that enter the first surface; theta [K, C] float64 or
    [M, K, C].  checkpoints [K + 1, 6, M] (see the module docstring)."""
    for k, (kind, deg, r_ap, eta, c0, k0) in enumerate(table):
        if checkpoints is not None:
            ck = checkpoints[k].double()
            o, d = _at(ck[:3].t(), o), _at(ck[3:].t(), d)
        row = theta[:, k].t() if theta.dim() == 3 else theta[k]
        o, d = surface_f64(o, d, row, kind, deg, r_ap, eta, c0, k0, trips[k])
    if checkpoints is not None:
        ck = checkpoints[len(table)].double()
        o, d = _at(ck[:3].t(), o), _at(ck[3:].t(), d)
    t = (d_sensor - o[:, 2]) / d[:, 2]
    return o + t.unsqueeze(-1) * d, d


def psf_f64(o, d, theta, table, trips, d_sensor, S, N, center, ps, ks, dp, checkpoints=None, ra=None, mask_dtype=torch.float32):
    """RAW (L, R) [N, ks, ks] float64 of point-major rays (ray (s, n) at n S + s) that are all alive at the sensor
    (ra: their weights, default 1): the trace, then splat_f64 with dp = (h, f, w, r) and the window test in mask_dtype.
    CPU tensors."""
    so, sd = trace_f64(o, d, theta, table, trips, d_sensor, checkpoints)
    sn = lambda v: v.reshape(N, S).t()
    ra = torch.ones(S, N, dtype=torch.float32) if ra is None else sn(ra)
    h, f, w, r = dp
    return splat_f64(sn(so[:, 0]), sn(so[:, 1]), sn(sd[:, 0]), sn(sd[:, 2]), ra, center, ps, ks, h, f, w, float(r),
                     mask_dtype=mask_dtype)
