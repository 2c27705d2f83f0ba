"""The layered render's backward restated in plain numpy from the text of the section ("For a live
ray", "Colour", "Coverage").  Nothing here comes from sdirt_amd.render_rt; the lookup's fp32 part is
tests/render_rt_f64.py's, as §7p's restatement takes it.  tests/test_render_layers_grad_cpu.py ties the product's own
restatement (layer_grads_float64) to this one, tests/test_gpu_render_layers_grad.py checks the kernel against it.

Every term is formed in float64 with one rounding per operation in the section's order, so it is the kernel's term in
every bit; only the order in which a texel's terms are added is free.  Per texel the function returns the gradient,
the number n of terms (those whose factor T_l is not 0: the others are exact zeros, issued or not) and sum|term| with
absolute values taken before any cancellation; bound() is the section's distance between two ways of adding them."""
import numpy as np

from render_rt_f64 import F32, _clamped, tap_origin


def taps(px, py, inv_texel, Ht, Wt):
    """-> idx [4, ...] int64 (offsets in the flattened plane, replicate addressing), w [4, ...] float64: w00, w01, w10, w11."""
    c0, r0, fu, fv = tap_origin(px, py, inv_texel, Ht, Wt)
    cl, cr, rt, rb = _clamped(c0, 0, Wt), _clamped(c0, 1, Wt), _clamped(r0, 0, Ht), _clamped(r0, 1, Ht)
    du, dv = fu.astype(np.float64), fv.astype(np.float64)
    idx = np.stack((rt * Wt + cl, rt * Wt + cr, rb * Wt + cl, rb * Wt + cr))
    w = np.stack(((1.0 - dv) * (1.0 - du), (1.0 - dv) * du, dv * (1.0 - du), dv * du))
    return idx, w


def read(planes, idx, w):
    """planes [N, Ht, Wt] -> [N, ...] float64: w00 v00 + w01 v01 + w10 v10 + w11 v11, left to right."""
    p = np.asarray(planes, F32).astype(np.float64).reshape(planes.shape[0], -1)
    t = w[0] * p[:, idx[0]]
    t = t + w[1] * p[:, idx[1]]
    t = t + w[2] * p[:, idx[2]]
    t = t + w[3] * p[:, idx[3]]
    return t


def layer_grads_f64(px, py, ra, w, alpha, tex, inv_texels, gnum):
    """px, py [L, S, H, W] fp32: every layer's landing point; ra [S, H, W]; w [V, S, H, W] fp32: the view weights;
    alpha [L, Ht, Wt] or None (every layer opaque); tex [L, T, Ht, Wt] or [T, Ht, Wt] shared; gnum [V, T, H, W] float64.
    -> dict of float64 / int64 arrays: galpha, n_alpha, abs_alpha [L, Ht, Wt] (None without alpha); gtex, n_tex, abs_tex
    of tex's shape; q [T, S, H, W], a, D, T_before [L, S, H, W] (per ray, for the tests that pick rays)."""
    ra, w = np.asarray(ra, F32), np.asarray(w, F32)
    tex = np.asarray(tex, F32)
    gnum = np.asarray(gnum, np.float64)
    L = len(inv_texels)
    shared = tex.ndim == 3
    NT, Ht, Wt = tex.shape[-3:]
    V = w.shape[0]
    live = ra != 0
    wr = np.where(live, w.astype(np.float64) * ra.astype(np.float64), 0.0)      # [V, S, H, W]
    q = wr[0] * gnum[0][:, None]                                                # side 0 first
    qa = wr[0] * np.abs(gnum[0])[:, None]
    if V == 2:
        q = q + wr[1] * gnum[1][:, None]
        qa = qa + wr[1] * np.abs(gnum[1])[:, None]
    out = {"gtex": np.zeros(tex.shape), "n_tex": np.zeros(tex.shape, np.int64), "abs_tex": np.zeros(tex.shape),
           "galpha": None, "n_alpha": None, "abs_alpha": None, "q": q}
    if alpha is not None:
        alpha = np.asarray(alpha, F32)
        out.update(galpha=np.zeros(alpha.shape), n_alpha=np.zeros(alpha.shape, np.int64), abs_alpha=np.zeros(alpha.shape))

    def scatter(name, where, idx, wj, val, aval, sel):
        for j in range(4):
            np.add.at(out["g" + name][where].reshape(-1), idx[j][sel], (val * wj[j])[sel])
            np.add.at(out["abs_" + name][where].reshape(-1), idx[j][sel], (aval * wj[j])[sel])
            np.add.at(out["n_" + name][where].reshape(-1), idx[j][sel], 1)

    T = np.ones(live.shape)
    kept = []
    for l in range(L):
        x = np.where(live, np.asarray(px[l], F32), F32(0))
        y = np.where(live, np.asarray(py[l], F32), F32(0))
        idx, wj = taps(x, y, inv_texels[l], Ht, Wt)
        a = np.ones(live.shape) if alpha is None else read(alpha[l:l + 1], idx, wj)[0]
        t = read(tex if shared else tex[l], idx, wj)
        g = T * a
        D, Dbar = q[0] * t[0], qa[0] * np.abs(t[0])
        for k in range(1, NT):
            D, Dbar = D + q[k] * t[k], Dbar + qa[k] * np.abs(t[k])
        sel = live & (T != 0)
        for k in range(NT):
            scatter("tex", (k,) if shared else (l, k), idx, wj, q[k] * g, qa[k] * g, sel)
        kept.append((idx, wj, a, D, Dbar, T))
        T = T * (1.0 - a)
    if alpha is not None:
        R, Rbar = np.zeros(live.shape), np.zeros(live.shape)
        for l in range(L - 1, -1, -1):
            idx, wj, a, D, Dbar, Tl = kept[l]
            d = D - R
            scatter("alpha", (l,), idx, wj, Tl * d, Tl * (Dbar + Rbar), live & (Tl != 0))
            R, Rbar = R + a * d, a * Dbar + (1.0 - a) * Rbar
    out["a"] = np.stack([k[2] for k in kept])
    out["D"] = np.stack([k[3] for k in kept])
    out["T_before"] = np.stack([k[5] for k in kept])
    return out


def bound(n, L, sum_abs):
    """§7q: per texel, the largest distance between two evaluations of the same n terms: 2 (n + 5 L + 22) 2^-53 sum|term|."""
    return 2.0 * (np.asarray(n, np.float64) + 5 * L + 22) * 2.0 ** -53 * sum_abs
