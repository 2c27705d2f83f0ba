"""A float64 torch restatement of the dual-pixel splat (monte_carlo.py:9-68, 135-240, 242-372), differentiable by
torch's own autograd: the yardstick of sdirt_forward_integral_grad.

Rays are given as the float32 arrays the kernels read (ox, oy, dx, dz, ra: [S, N]); the window test runs in
`mask_dtype` (float32: the kernels' decision; float64: a reference run on float64 rays), everything else in float64.
h, f, w broadcast against [S, N] and the centres against [S, N, 2]: pass per-ray leaves to get per-ray gradient
terms.  The segment area A(x) = r^2 (u - sin(2u) / 2), u = acos(x / r), is differentiated by its chord
-2 sqrt(r^2 - x^2) (SegArea), which is finite where acos' derivative is not (|x| = r).

The kernel takes its clamp and cell decisions on fp32 values, this file in float64: fragile_rays names the rays that
sit within rounding of a decision at which the derivative jumps, which no float64 reference can judge.
"""
import math

import torch


class SegArea(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r):
        ctx.save_for_backward(x)
        ctx.r = r
        u = torch.acos(x / r)
        return r * r * (u - 0.5 * torch.sin(2 * u))

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        r = ctx.r
        return g * (-2.0 * torch.sqrt(torch.clamp((r - x) * (r + x), min=0.0))), None


def sub_pixel_areas(t, h, f, w, r):
    """(s_l, s_r) per ray for x_tan = t: the small-r model (r <= 0.5) or the big-r one."""
    def lens_x(a):          # sub-pixel boundary a*w projected through the microlens
        return a * w - (f * t - a * w) * h / (f - h)

    def margin_x(a):
        return a * w - h * t

    Z = {}
    for a in (1.0, 0.0, -1.0):
        if r <= 0.5:
            c1 = torch.clamp(lens_x(a), -r, r)
            c2 = torch.clamp(margin_x(a), -0.5, 0.5)
            Z[a] = SegArea.apply(c1, r) - c2 - SegArea.apply(torch.clamp(c2, -r, r), r)
        else:
            tr = math.asin(0.5 / r)
            tl = math.pi - tr

            def T(x):       # area under the microlens, minus its part outside the pixel (u outside [tr, tl])
                c = torch.clamp(x, -0.5, 0.5)
                ue = torch.clamp(torch.acos(c / r), tr, tl)
                return SegArea.apply(c, r) - r * r * (ue - 0.5 * torch.sin(2 * ue)) - r * torch.cos(ue)
            c2 = torch.clamp(margin_x(a), -0.5, 0.5)
            Z[a] = T(lens_x(a)) - c2 - T(margin_x(a))
    return Z[-1.0] - Z[0.0], Z[0.0] - Z[1.0]


def boundaries(t, h, f, w):
    """(x1, x2), each [3, ...]: the lens-projected and the margin sub-pixel boundaries for a = +1, 0, -1."""
    x1 = torch.stack([a * w - (f * t - a * w) * h / (f - h) + 0 * t for a in (1.0, 0.0, -1.0)])
    x2 = torch.stack([a * w - h * t + 0 * t for a in (1.0, 0.0, -1.0)])
    return x1, x2


def fragile_x(t, h, f, w, r, band=1e-5):
    """Whether x_tan = t puts a sub-pixel boundary within `band` of a clamp edge at which d(s_l, s_r)/d(h, f, w) JUMPS:
    |x2| = 0.5 (both models: -1 - A'(x2) inside, 0 outside) and, for r > 0.5, |x1| = 0.5 (-1 or A'(x1) inside, 0
    outside).  No jump at |x| = r (the chord is 0 there) nor at the u clamp |c| = sqrt(r^2 - 1/4) (the chord is -1
    there, the open branch's value)."""
    x1, x2 = boundaries(torch.as_tensor(t).double(), h, f, w)
    bad = ((x2.abs() - 0.5).abs() < band).any(0)
    if r > 0.5:
        bad = bad | ((x1.abs() - 0.5).abs() < band).any(0)
    return bad


def gate_states(t, h, f, w, r):
    """The clamp gates of the derivative per (boundary, ray), from float64 quantities: name -> (open, closed), bool
    [3, ...].  A gate nested in another one (gi and u2 inside g2, u1 inside g1) counts, open or closed, only where
    the outer gate passes the gradient: elsewhere its state changes nothing.
    gi is reported for completeness only: the kernel's chord() clamps (r - x)(r + x) at 0, so beyond |x2| = r the
    term gi switches off is 0 already, and a kernel with gi stuck open computes the same numbers.  A coverage
    figure for gi therefore says where the rays went, not that a wrong gi would be noticed."""
    x1, x2 = boundaries(torch.as_tensor(t).double(), h, f, w)
    g2 = x2.abs() <= 0.5
    if r <= 0.5:
        g1, gi = x1.abs() <= r, x2.abs() <= r
        return {"g1": (g1, ~g1), "g2": (g2, ~g2), "gi": (g2 & gi, g2 & ~gi)}
    g1, edge = x1.abs() <= 0.5, math.sqrt(r * r - 0.25)
    u1, u2 = x1.abs() <= edge, x2.abs() <= edge
    return {"g1": (g1, ~g1), "g2": (g2, ~g2), "u1": (g1 & u1, g1 & ~u1), "u2": (g2 & u2, g2 & ~u2)}


def _window(ox, oy, ra, center, ps, ks, mask_dtype):
    """ra * (the ray is inside the window), float64 [S, N]: monte_carlo.py:37 in mask_dtype on the kernel's values."""
    hi = (ks / 2 - 0.5) * ps
    cm = center.detach().to(mask_dtype)
    pxm, pym = (-ox.to(mask_dtype)) - cm[..., 0], (-oy.to(mask_dtype)) - cm[..., 1]
    lim = torch.tensor(hi - 0.01 * ps, dtype=mask_dtype)
    return ra.double() * ((pxm.abs() < lim) & (pym.abs() < lim)).double()


def _centres(center, S, N):
    center = torch.as_tensor(center)
    return center.expand(S, N, 2) if center.dim() == 3 else center.unsqueeze(0).expand(S, N, 2)


def live_in_window(ox, oy, ra, center, ps, ks):
    """bool [S, N]: the rays that carry weight into the grids (ra != 0 and inside the kernel's fp32 window)."""
    S, N = ox.shape
    return _window(ox, oy, ra, _centres(center, S, N), ps, ks, torch.float32) != 0


def fragile_rays(ox, oy, dx, dz, ra, center, ps, ks, h, f, w, r, x_band=1e-5, cell_band=None):
    """bool [S, N]: the live, in-window rays within rounding of a decision at which the gradient jumps, so that the
    kernel (fp32 decisions) and a float64 reference may legitimately fall on different sides:
      * a jump boundary of fragile_x within x_band = 1e-5 in x (O(1) quantities out of a handful of fp32
        operations: about 100 x their rounding);
      * a pixel-cell boundary of rowf / colf within cell_band = 8 ks 2^-23 pixels (the fraction is what is left of
        an fp32 number of size <= ks after a subtraction, a division and a product); the cell decides the slope of
        g . taps, so the centre gradients.
    The window edge is no such decision: splat_f64 tests it in fp32 with the kernel's own operations."""
    S, N = ox.shape
    if cell_band is None:
        cell_band = 8 * ks * 2.0 ** -23
    center = _centres(center, S, N)
    hi, lo = (ks / 2 - 0.5) * ps, (-ks / 2 + 0.5) * ps
    wgt = _window(ox, oy, ra, center, ps, ks, torch.float32)
    keep = wgt != 0
    rowf = (((-oy.double()) - center[..., 1].double()) * wgt - hi) / (lo - hi) * (ks - 1)        # :38, the weight too
    colf = (((-ox.double()) - center[..., 0].double()) * wgt - lo) / (hi - lo) * (ks - 1)
    cell = ((rowf - torch.round(rowf)).abs() < cell_band) | ((colf - torch.round(colf)).abs() < cell_band)
    t = -dx.double() / dz.double()
    return keep & (cell | fragile_x(t, float(h), float(f), float(w), r, x_band))


def _fractions_fp32(ox, oy, center, keep, ps, ks):
    """(rowf, colf) as grad_taps / splat_taps compute them: fp32, the kernel's constants and operation order."""
    hi, lo = (ks / 2 - 0.5) * ps, (-ks / 2 + 0.5) * ps
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    c, wgt = center.detach().float(), keep.float()
    px = ((-ox) - c[..., 0]) * wgt
    py = ((-oy) - c[..., 1]) * wgt
    return ((py - f32(hi)) / f32(lo - hi)) * f32(ks - 1), ((px - f32(lo)) / f32(hi - lo)) * f32(ks - 1)


def splat_f64(ox, oy, dx, dz, ra, center, ps, ks, h, f, w, r, mask_dtype=torch.float32, frac_dtype=torch.float64):
    """RAW (L, R) [N, ks, ks] float64.  ox.. : float32 [S, N]; center [N, 2] or [S, N, 2].
    frac_dtype=torch.float32: the values of the bilinear fractions (and the cells) are the kernel's fp32 ones,
    widened; their derivative by the centres stays the float64 one."""
    S, N = ox.shape
    center = _centres(center, S, N)
    hi, lo = (ks / 2 - 0.5) * ps, (-ks / 2 + 0.5) * ps
    keep = _window(ox, oy, ra, center, ps, ks, mask_dtype)
    px = ((-ox.double()) - center[..., 0].double()) * keep
    py = ((-oy.double()) - center[..., 1].double()) * keep
    rowf = (py - hi) / (lo - hi) * (ks - 1)
    colf = (px - lo) / (hi - lo) * (ks - 1)
    if frac_dtype == torch.float32:
        row32, col32 = _fractions_fp32(ox, oy, center, keep, ps, ks)
        rowf = row32.double() + (rowf - rowf.detach())
        colf = col32.double() + (colf - colf.detach())
    elif frac_dtype != torch.float64:
        raise ValueError("frac_dtype must be torch.float64 or torch.float32")
    r0, c0 = torch.floor(rowf).detach(), torch.floor(colf).detach()
    wb, wr = rowf - r0, colf - c0
    r0, c0 = r0.long(), c0.long()
    t = -dx.double() / dz.double()
    sl, sr = sub_pixel_areas(t, h, f, w, r)
    sl, sr = sl.expand(S, N), sr.expand(S, N)
    n_idx = torch.arange(N).unsqueeze(0).expand(S, N)
    out = []
    for s in (sl, sr):
        g = torch.zeros(N * ks * ks, dtype=torch.float64)
        for dr_, dc_, wt in ((0, 0, (1 - wb) * (1 - wr)), (0, 1, (1 - wb) * wr), (1, 0, wb * (1 - wr)), (1, 1, wb * wr)):
            idx = (n_idx * ks + (r0 + dr_).clamp(0, ks - 1)) * ks + (c0 + dc_).clamp(0, ks - 1)
            g = g.index_add(0, idx.reshape(-1), (wt * keep * s).reshape(-1))
        out.append(g.reshape(N, ks, ks))
    return out[0], out[1]


def max_normalise(psf):
    """optics.py:983-987."""
    N = psf.shape[0]
    return psf / (psf.reshape(N, -1).max(dim=-1).values.reshape(N, 1, 1) + 1e-6)
