"""Ray-traced layered render: lookup per layer, compositing per ray and the sums restated in plain
numpy from the text of the section ("Lookup per layer", "Compositing per ray", "Sums").  Nothing here comes from
sdirt_amd.render_rt; the lookup's fp32 part is tests/render_rt_f64.py's (the section takes it from §7o).
tests/test_render_layers_cpu.py ties the product's own restatement (layer_sums_float64) to this one on synthetic
landings, tests/test_gpu_render_layers.py checks the kernel's sums against it.

Every per-ray quantity (a_l, t_{l,k}, g, c_k, T, o, wr, the three terms) is the kernel's in every bit: float64, one
rounding per operation, in the section's order; only the order of the sum over s is free.  Two sums of the same S
float64 terms differ by at most 2 S 2^-53 sum|term| (render_rt_f64's docstring)."""
import numpy as np

from render_rt_f64 import F32, _clamped, sum_bound, tap_origin  # noqa: F401  (sum_bound: for the importing tests)


def lookup(planes, px, py, inv_texel):
    """§7o's lookup of planes [N, Ht, Wt] fp32 at px, py [S, H, W] fp32 (finite) with inv_texel texels per mm
    -> [N, S, H, W] float64: w00 v00 + w01 v01 + w10 v10 + w11 v11, summed left to right."""
    planes = np.asarray(planes, F32)
    _, Ht, Wt = planes.shape
    c0, r0, fu, fv = tap_origin(px, py, inv_texel, Ht, Wt)
    cl, cr, rt, rb = _clamped(c0, 0, Wt), _clamped(c0, 1, Wt), _clamped(r0, 0, Ht), _clamped(r0, 1, Ht)
    du, dv = fu.astype(np.float64), fv.astype(np.float64)
    p64 = planes.astype(np.float64)
    t = ((1.0 - dv) * (1.0 - du)) * p64[:, rt, cl]
    t = t + ((1.0 - dv) * du) * p64[:, rt, cr]
    t = t + (dv * (1.0 - du)) * p64[:, rb, cl]
    t = t + (dv * du) * p64[:, rb, cr]
    return t


def composite(px, py, ra, alpha, tex, inv_texels):
    """px, py [L, S, H, W] fp32: every layer's landing point; ra [S, H, W]; alpha [L, Ht, Wt]; tex [L, T, Ht, Wt] or
    [T, Ht, Wt] shared by all layers -> c [T, S, H, W], o [S, H, W], a [L, S, H, W] (the coverage read on every layer)
    and T_before [L, S, H, W] (the transmittance a layer is met with), float64; dead rays (ra == 0) are given the
    point (0, 0) to look up and are left out by the caller."""
    alpha, tex = np.asarray(alpha, F32), np.asarray(tex, F32)
    L = alpha.shape[0]
    if tex.ndim == 3:
        tex = np.broadcast_to(tex, (L,) + tex.shape)
    live = np.asarray(ra, F32) != 0
    T = np.ones(live.shape)
    c = np.zeros((tex.shape[1],) + live.shape)
    a_all, T_before = np.zeros((L,) + live.shape), np.zeros((L,) + live.shape)
    for l in range(L):
        x = np.where(live, np.asarray(px[l], F32), F32(0))
        y = np.where(live, np.asarray(py[l], F32), F32(0))
        a = lookup(alpha[l:l + 1], x, y, inv_texels[l])[0]
        t = lookup(tex[l], x, y, inv_texels[l])
        a_all[l], T_before[l] = a, T
        g = T * a
        c = c + g * t
        T = T * (1.0 - a)
    return c, 1.0 - T, a_all, T_before


def layer_sums_f64(px, py, ra, w, alpha, tex, inv_texels):
    """-> num [V, T, H, W], den [V, H, W], cov [V, H, W], sum|wr c_k| [V, T, H, W], sum|wr o| [V, H, W], float64,
    the samples summed in order.  w [V, S, H, W] fp32: the view weights of every ray."""
    ra, w = np.asarray(ra, F32), np.asarray(w, F32)
    live = ra != 0
    c, o, _, _ = composite(px, py, ra, alpha, tex, inv_texels)
    wr = np.where(live, w.astype(np.float64) * ra.astype(np.float64), 0.0)      # [V, S, H, W]
    terms = np.where(live, wr[:, None] * c[None], 0.0)                          # [V, T, S, H, W]
    oterms = np.where(live, wr * o[None], 0.0)                                  # [V, S, H, W]
    S = ra.shape[0]
    num, den = np.zeros(terms.shape[:2] + terms.shape[3:]), np.zeros(wr.shape[:1] + wr.shape[2:])
    cov, ab, oab = np.zeros_like(den), np.zeros_like(num), np.zeros_like(den)
    for s in range(S):
        num += terms[:, :, s]
        den += wr[:, s]
        cov += oterms[:, s]
        ab += np.abs(terms[:, :, s])
        oab += np.abs(oterms[:, s])
    return num, den, cov, ab, oab


def stack_classes(ra, a_all, T_before):
    """Shares of the live rays: a_0 == 0, 0 < a_0 < 1, a_0 == 1, T == 0 reached before the last layer, T never 0."""
    live = np.asarray(ra, F32) != 0
    a0 = a_all[0][live]
    T_after_last = (T_before[-1] * (1.0 - a_all[-1]))[live]
    early = (T_before[-1][live] == 0) if a_all.shape[0] > 1 else np.zeros(a0.shape, bool)
    return {"a0=0": float((a0 == 0).mean()), "0<a0<1": float(((a0 > 0) & (a0 < 1)).mean()),
            "a0=1": float((a0 == 1).mean()), "T=0 early": float(early.mean()),
            "T never 0": float((T_after_last != 0).mean())}
