"""Ray-traced plane render: the lookup and the sums restated in plain numpy from the text of the
section ("Lookup", "Sums"), and the float64 closed form of the dual-pixel weights.  Nothing here comes from
sdirt_amd.render_rt: tests/test_render_rt_f64_cpu.py ties the product's own restatement (plane_sums_float64) to this
one on synthetic landings, tests/test_gpu_render_raytraced_edges.py checks the kernel's sums against it.

The order of operations is the section's: the lookup in fp32 with one rounding per operation (numpy float32 arrays
round every elementwise operation once), the four bilinear products and their sum in float64 from left to right, then
(w ra) times that.  So every term is the kernel's term in every bit and only the order of the sum over s is free: two
sums of the same S float64 terms differ by at most 2 S 2^-53 sum|term| (each is within (S - 1) 2^-53 sum|term| of the
exact sum to first order; the factor 2 S leaves room for the second-order terms)."""
import numpy as np

F32 = np.float32


def tap_origin(px, py, inv_texel, Ht, Wt):
    """The fp32 part of the lookup: -> (c0, r0, fu, fv) float32, c0 / r0 the UNCLAMPED column / row of the top-left
    tap (integers held in fp32).  u = Wt/2 - px inv, v = Ht/2 + py inv, a = u - 0.5, b = v - 0.5, floor, a - c0."""
    px, py = np.asarray(px, F32), np.asarray(py, F32)
    inv = F32(inv_texel)
    with np.errstate(invalid="ignore", over="ignore"):
        u = F32(Wt) * F32(0.5) - px * inv
        v = F32(Ht) * F32(0.5) + py * inv
        a, b = u - F32(0.5), v - F32(0.5)
        c0, r0 = np.floor(a), np.floor(b)
        fu, fv = a - c0, b - r0
    assert u.dtype == v.dtype == fu.dtype == fv.dtype == F32
    return c0, r0, fu, fv


def tap_classes(first, n, live):
    """Shares of the live rays whose first tap index is < 0 (both taps on the near edge texel or beyond it),
    in 0 .. n-2 (two distinct texels) and >= n - 1 (the far edge): (lo, mid, hi), summing to 1."""
    f = np.asarray(first, np.float64)[live]
    return float((f < 0).mean()), float(((f >= 0) & (f < n - 1)).mean()), float((f >= n - 1).mean())


def _clamped(first, off, n):
    """Replicate addressing: index first + off clamped to [0, n - 1] (the clamp is applied in float64, where every
    fp32 integer and its successor are exact)."""
    return np.clip(np.asarray(first, np.float64) + off, 0, n - 1).astype(np.int64)


def plane_sums_f64(px, py, ra, w, tex, inv_texel):
    """px, py, ra [S, H, W] fp32 (the landing point on the plane and the ray's validity), w [V, S, H, W] fp32 (the
    view weights of every ray), tex [T, Ht, Wt] fp32, inv_texel: texels per mm (rounded to fp32 as the kernel's argument).
    -> num [V, T, H, W], den [V, H, W], sum|term| [V, T, H, W], float64.  A ray with ra == 0 contributes to nothing,
    whatever its landing point holds (NaN, +-inf)."""
    ra = np.asarray(ra, F32)
    w = np.asarray(w, F32)
    tex = np.asarray(tex, F32)
    T, Ht, Wt = tex.shape
    live = ra != 0
    px = np.where(live, np.asarray(px, F32), F32(0))           # a dead ray gets a point to look up and is left out below
    py = np.where(live, np.asarray(py, F32), F32(0))
    c0, r0, fu, fv = tap_origin(px, py, inv_texel, Ht, Wt)
    cl, cr, rt, rb = _clamped(c0, 0, Wt), _clamped(c0, 1, Wt), _clamped(r0, 0, Ht), _clamped(r0, 1, Ht)
    du, dv = fu.astype(np.float64), fv.astype(np.float64)
    t64 = tex.astype(np.float64)
    t = ((1.0 - dv) * (1.0 - du)) * t64[:, rt, cl]             # [T, S, H, W], left to right as the section writes it
    t = t + ((1.0 - dv) * du) * t64[:, rt, cr]
    t = t + (dv * (1.0 - du)) * t64[:, rb, cl]
    t = t + (dv * du) * t64[:, rb, cr]
    wr = np.where(live, w.astype(np.float64) * ra.astype(np.float64), 0.0)      # [V, S, H, W]
    terms = np.where(live, wr[:, None] * t[None], 0.0)         # [V, T, S, H, W]
    S = ra.shape[0]
    num, den = np.zeros(terms.shape[:2] + terms.shape[3:]), np.zeros(wr.shape[:1] + wr.shape[2:])
    ab = np.zeros_like(num)
    for s in range(S):                                         # the sample order
        num += terms[:, :, s]
        den += wr[:, s]
        ab += np.abs(terms[:, :, s])
    return num, den, ab


def sum_bound(S):
    """Relative to sum|term|: the largest distance between two orders of summing the same S float64 terms."""
    return 2 * S * 2.0 ** -53


def weights_f64(x, h, f, w, r):
    """(sl, sr) of monte_carlo.py:170-203 (the small-radius model, r <= 0.5) in float64, literally: clamp, arccos,
    u - sin(2u) / 2."""
    x = np.asarray(x, np.float64)

    def area(a, b):                                    # of the circle of radius r between abscissae a <= b
        ua, ub = np.arccos(np.clip(a, -r, r) / r), np.arccos(np.clip(b, -r, r) / r)
        return r * r * ((ua - np.sin(2 * ua) / 2) - (ub - np.sin(2 * ub) / 2))

    fx, fmh = f * x, f - h
    xr, xm, xl = w - (fx - w) * h / fmh, -fx * h / fmh, -w - (fx + w) * h / fmh      # through the microlens
    sr_ml, sl_ml = area(xm, xr), area(xl, xm)
    xr, xm, xl = (np.clip(v, -0.5, 0.5) for v in (w - h * x, -h * x, -w - h * x))    # straight onto the pixel
    sr_mg, sl_mg = (xr - xm) - area(xm, xr), (xm - xl) - area(xl, xm)
    return sl_ml + sl_mg, sr_ml + sr_mg
