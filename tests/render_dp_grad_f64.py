"""The layered render's backward into the dual-pixel parameters h, f, w, restated from the text of the
section.  Nothing here comes from sdirt_amd.render_rt.  It combines
  the lookup of tests/render_rt_f64.py (through tests/render_layers_f64.lookup),
  the composite of tests/render_layers_f64.py, with the forward's walk as §7r states it: it stops where T reaches 0,
  so a layer behind an opaque texel is not read, whatever its texture holds,
  sub_pixel_areas of tests/splat_f64.py (which tests/test_dp_grad_cpu.py holds against the reference's own autograd),
  differentiated through per-ray leaves as tests/energy_f64.energy_grad_f64 does.

Per live ray: A_side = ra (gnum[side, 0] c_0 + ... + gnum[side, T-1] c_{T-1} + gden[side]), left to right with gden
last; the views are (w_L, w_R) = (s_r, s_l); the ray's term in theta_j is A_0 dw_L/dtheta_j + A_1 dw_R/dtheta_j.  The
clamp decisions are taken in float64 at the given x_tan (the kernel takes them on fp32 values: splat_f64.fragile_x
names the rays no float64 reference can judge)."""
import numpy as np
import torch

from render_layers_f64 import lookup
from render_rt_f64 import F32
from splat_f64 import sub_pixel_areas


def composite_to_t0(px, py, ra, alpha, tex, inv_texels):
    """§7p's composite with the walk of the forward: px, py [L, S, H, W] fp32, ra [S, H, W], alpha [L, Ht, Wt] or None
    (every layer opaque), tex [L, T, Ht, Wt] or [T, Ht, Wt] -> c [T, S, H, W] float64 and the number of layers every
    ray read [S, H, W]."""
    tex = np.asarray(tex, F32)
    L = len(inv_texels)
    if tex.ndim == 3:
        tex = np.broadcast_to(tex, (L,) + tex.shape)
    live = np.asarray(ra, F32) != 0
    T = np.ones(live.shape)
    c = np.zeros((tex.shape[1],) + live.shape)
    read = np.zeros(live.shape, np.int64)
    for l in range(L):
        reads = live & (T != 0)
        x = np.where(reads, np.asarray(px[l], F32), F32(0))
        y = np.where(reads, np.asarray(py[l], F32), F32(0))
        a = np.ones(live.shape) if alpha is None else lookup(np.asarray(alpha, F32)[l:l + 1], x, y, inv_texels[l])[0]
        with np.errstate(invalid="ignore"):
            t = lookup(tex[l], x, y, inv_texels[l])
            g = T * a
            c = np.where(reads, c + g * t, c)
        T = np.where(reads, T * (1.0 - a), T)
        read += reads
    return c, read


def dp_grads_f64(px, py, ra, x_tan, alpha, tex, inv_texels, gnum, gden, h, f, w, r):
    """x_tan [S, H, W] fp32; gnum [2, T, H, W], gden [2, H, W] or None, float64.
    -> dict: grad [3] (h, f, w), scale [3] = the sums of |A_0 dw_L| + |A_1 dw_R| (magnitudes before any cancellation),
    n = the number of rays with a term, A [2, S, H, W], read [S, H, W]."""
    ra = np.asarray(ra, F32)
    live = ra != 0
    gnum = np.asarray(gnum, np.float64)
    c, read = composite_to_t0(px, py, ra, alpha, tex, inv_texels)
    A = []
    for side in range(2):
        s = gnum[side, 0] * c[0]
        for k in range(1, c.shape[0]):
            s = s + gnum[side, k] * c[k]
        if gden is not None:
            s = s + np.asarray(gden, np.float64)[side]
        with np.errstate(invalid="ignore"):
            A.append(np.where(live, ra.astype(np.float64) * s, 0.0))
    A = np.stack(A)
    t = torch.from_numpy(np.where(live, np.asarray(x_tan, F32), F32(0)).astype(np.float64))
    per_side = []
    for side in range(2):
        hv, fv, wv = (torch.full(t.shape, float(v), dtype=torch.float64, requires_grad=True) for v in (h, f, w))
        sl, sr = sub_pixel_areas(t, hv, fv, wv, r)
        (torch.from_numpy(A[side]) * (sr if side == 0 else sl)).sum().backward()
        per_side.append(torch.stack([torch.zeros_like(t) if v.grad is None else v.grad for v in (hv, fv, wv)]))
    terms = per_side[0] + per_side[1]                                              # [3, S, H, W]
    mags = per_side[0].abs() + per_side[1].abs()
    return dict(grad=terms.flatten(1).sum(1).numpy(), scale=mags.flatten(1).sum(1).numpy(),
                n=int((live & ((A[0] != 0) | (A[1] != 0))).sum()), A=A, read=read)
