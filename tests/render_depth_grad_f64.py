"""The layered render's backward into the layer depths and texel scales restated in plain numpy from
the text of the section.  Nothing here comes from sdirt_amd.render_rt.  It combines
  the lookup of tests/render_rt_f64.py (tap_origin: the fp32 steps, the floor decisions and the two fractions),
  the taps, the reads and the compositing adjoint of tests/render_layers_grad_f64.py (q, a_l, D_l, T_l per ray),
  the derivative of a lookup in (fu, fv) from its four taps, and the ray's slopes sx = dx / dz, sy = dy / dz.

Every term is formed in float64 with one rounding per operation in the section's order; only the order of the sum over
the rays is free.  Per layer and component the function returns the gradient, the number n of terms (the live rays
whose T_l is not 0) and sum|term| with absolute values taken before any cancellation; bound() is the section's distance
between two evaluations."""
import numpy as np

import render_layers_grad_f64 as RG
from render_rt_f64 import F32, tap_origin


def rho(L):
    """§7s: the roundings one term carries at most, for NT <= 4: 5 L + 21 for e_l (§7q's count without its three
    final products plus d and T d), 6 for a lookup's derivative, 1 for e da, 1 for the sum that makes Pu, 1 for sx,
    3 for Pv sy - Pu sx and 1 for the factor inv_l: 5 L + 33.  (The colour half of Pu carries fewer: 2 L + 23.)"""
    return 5 * L + 33


def bound(n, L, sum_abs):
    """§7s: per layer and component, the largest distance between two evaluations of the same n terms."""
    return 2.0 * (np.asarray(n, np.float64) + rho(L)) * 2.0 ** -53 * np.asarray(sum_abs, np.float64)


def slopes(planes, idx, fu, fv, magnitudes=False):
    """d/dfu, d/dfv of RG.read(planes, idx, w): (1 - fv)(v01 - v00) + fv (v11 - v10), (1 - fu)(v10 - v00) + fu (v11 - v01)
    -> two [N, ...] float64.  magnitudes: with |v01 - v00|, ... instead (nothing cancels)."""
    p = np.asarray(planes, F32).astype(np.float64).reshape(planes.shape[0], -1)
    v00, v01, v10, v11 = (p[:, idx[j]] for j in range(4))
    with np.errstate(invalid="ignore"):
        top, bottom, left, right = v01 - v00, v11 - v10, v10 - v00, v11 - v01
        if magnitudes:
            top, bottom, left, right = np.abs(top), np.abs(bottom), np.abs(left), np.abs(right)
        return (1.0 - fv) * top + fv * bottom, (1.0 - fu) * left + fu * right


def depth_grads_f64(px, py, ra, w, dirs, alpha, tex, inv_texels, gnum):
    """px, py [L, S, H, W] fp32: every layer's landing point; ra [S, H, W]; w [V, S, H, W] fp32: the view weights;
    dirs [3, S, H, W] fp32: dx, dy, dz of every ray after the trace; alpha [L, Ht, Wt] or None (every layer opaque:
    the ray meets layer 0 only); tex [L, T, Ht, Wt] or [T, Ht, Wt] shared; gnum [V, T, H, W] float64.
    -> dict: grad [L, 2] (the gradient in depth_l and in inv_texel_l), n [L], abs [L, 2], and per ray [L, S, H, W]:
    Pu, Pv, cov_u = e_l da_l/dfu, col_u = g_l sum_k q_k dt_{l,k}/dfu, a, T_before, c0 (the unclamped first column)."""
    ra = np.asarray(ra, F32)
    tex = np.asarray(tex, F32)
    gnum = np.asarray(gnum, np.float64)
    dirs = np.asarray(dirs, F32)
    L = len(inv_texels)
    shared = tex.ndim == 3
    NT, Ht, Wt = tex.shape[-3:]
    live = ra != 0
    met = 1 if alpha is None else L                             # an opaque layer 0 leaves T = 0: nothing behind is read
    base = RG.layer_grads_f64(px[:met], py[:met], ra, w, None if alpha is None else np.asarray(alpha, F32)[:met],
                              tex if shared else tex[:met], list(inv_texels)[:met], gnum)
    q, a_all, D_all, T_all = base["q"], base["a"], base["D"], base["T_before"]
    wr = np.where(live, np.asarray(w, F32).astype(np.float64) * ra.astype(np.float64), 0.0)
    qa = wr[0] * np.abs(gnum[0])[:, None]
    if wr.shape[0] == 2:
        qa = qa + wr[1] * np.abs(gnum[1])[:, None]
    dz = np.where(live, dirs[2].astype(np.float64), 1.0)
    sx = np.where(live, dirs[0].astype(np.float64) / dz, 0.0)
    sy = np.where(live, dirs[1].astype(np.float64) / dz, 0.0)
    out = {k: np.zeros((L,) + live.shape) for k in ("Pu", "Pv", "cov_u", "col_u", "a", "T_before", "c0")}
    grad, mags, n = np.zeros((L, 2)), np.zeros((L, 2)), np.zeros(L, np.int64)
    R, Rbar = np.zeros(live.shape), np.zeros(live.shape)
    for l in range(met - 1, -1, -1):
        x = np.where(live, np.asarray(px[l], F32), F32(0))
        y = np.where(live, np.asarray(py[l], F32), F32(0))
        idx, wj = RG.taps(x, y, inv_texels[l], Ht, Wt)
        c0, _, fu, fv = tap_origin(x, y, inv_texels[l], Ht, Wt)
        fu, fv = fu.astype(np.float64), fv.astype(np.float64)
        planes = tex if shared else tex[l]
        t = RG.read(planes, idx, wj)
        tu, tv = slopes(planes, idx, fu, fv)
        tua, tva = slopes(planes, idx, fu, fv, magnitudes=True)
        Dbar = qa[0] * np.abs(t[0])
        Cu, Cv, Cua, Cva = q[0] * tu[0], q[0] * tv[0], qa[0] * tua[0], qa[0] * tva[0]
        for k in range(1, NT):
            Dbar = Dbar + qa[k] * np.abs(t[k])
            Cu, Cv, Cua, Cva = Cu + q[k] * tu[k], Cv + q[k] * tv[k], Cua + qa[k] * tua[k], Cva + qa[k] * tva[k]
        if alpha is None:
            au = av = aua = ava = np.zeros(live.shape)
        else:
            (au,), (av,) = slopes(np.asarray(alpha, F32)[l:l + 1], idx, fu, fv)
            (aua,), (ava,) = slopes(np.asarray(alpha, F32)[l:l + 1], idx, fu, fv, magnitudes=True)
        a, D, Tl = a_all[l], D_all[l], T_all[l]
        d = D - R
        e, g, eb = Tl * d, Tl * a, Tl * (Dbar + Rbar)
        Pu, Pv = e * au + g * Cu, e * av + g * Cv
        Pua, Pva = eb * aua + g * Cua, eb * ava + g * Cva
        inv = np.float64(F32(inv_texels[l]))
        sel = live & (Tl != 0)
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        terms = (inv * (Pv * sy - Pu * sx), Pv * y64 - Pu * x64)
        tabs = (inv * (Pva * np.abs(sy) + Pua * np.abs(sx)), Pva * np.abs(y64) + Pua * np.abs(x64))
        for comp in range(2):
            lane = np.zeros(live.shape[1:])
            for s in range(live.shape[0]):                      # a lane's samples in order, then the lanes
                lane += np.where(sel[s], terms[comp][s], 0.0)
            grad[l, comp] = lane.sum()
            mags[l, comp] = np.where(sel, tabs[comp], 0.0).sum()
        n[l] = int(sel.sum())
        out["Pu"][l], out["Pv"][l] = np.where(sel, Pu, 0.0), np.where(sel, Pv, 0.0)
        out["cov_u"][l], out["col_u"][l] = np.where(sel, e * au, 0.0), np.where(sel, g * Cu, 0.0)
        out["a"][l], out["T_before"][l], out["c0"][l] = a, Tl, c0
        R, Rbar = R + a * d, a * Dbar + (1.0 - a) * Rbar
    out.update(grad=grad, abs=mags, n=n)
    return out
