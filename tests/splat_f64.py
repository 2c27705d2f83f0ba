"""A float64 torch restatement of the dual-pixel splat (monte_carlo.py:9-68, 135-240, 242-372), differentiable by
torch's own autograd: the yardstick of sdirt_forward_integral_grad.

Rays are given as the float32 arrays the kernels read (ox, oy, dx, dz, ra: [S, N]); the window test runs in
`mask_dtype` (float32: the kernels' decision; float64: a reference run on float64 rays), everything else in float64.
h, f, w broadcast against [S, N] and the centres against [S, N, 2]: pass per-ray leaves to get per-ray gradient
terms.  The segment area A(x) = r^2 (u - sin(2u) / 2), u = acos(x / r), is differentiated by its chord
-2 sqrt(r^2 - x^2) (SegArea), which is finite where acos' derivative is not (|x| = r).
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


def splat_f64(ox, oy, dx, dz, ra, center, ps, ks, h, f, w, r, mask_dtype=torch.float32):
    """RAW (L, R) [N, ks, ks] float64.  ox.. : float32 [S, N]; center [N, 2] or [S, N, 2]."""
    S, N = ox.shape
    center = torch.as_tensor(center).expand(S, N, 2) if torch.as_tensor(center).dim() == 3 else \
        torch.as_tensor(center).unsqueeze(0).expand(S, N, 2)
    hi, lo = (ks / 2 - 0.5) * ps, (-ks / 2 + 0.5) * ps
    # window test (monte_carlo.py:37) in mask_dtype, on the values the kernel sees
    cm = center.detach().to(mask_dtype)
    pxm, pym = (-ox.to(mask_dtype)) - cm[..., 0], (-oy.to(mask_dtype)) - cm[..., 1]
    lim = torch.tensor(hi - 0.01 * ps, dtype=mask_dtype)
    keep = ra.double() * ((pxm.abs() < lim) & (pym.abs() < lim)).double()
    px = ((-ox.double()) - center[..., 0].double()) * keep
    py = ((-oy.double()) - center[..., 1].double()) * keep
    rowf = (py - hi) / (lo - hi) * (ks - 1)
    colf = (px - lo) / (hi - lo) * (ks - 1)
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
