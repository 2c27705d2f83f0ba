"""The render of a dual-pixel pair from a PSF volume restated in torch (float64 on the CPU by default), for the tests
of sdirt_render_volume.hip.  Not a test file.

    K[b,y,x]  = sum over the 8 corners of w * V[corner]             w = wz * wy * wx, each factor f or 1 - f
    out_s     = render_f64(img, K)                                  (tests/render_f64.py: same flip, same padding)
    dV[node]  = sum_{b,y,x} w(b,y,x; node) * sum_c G_s[b,c,y,x] * P[b,c,(y,x) + (ks-1-i, ks-1-j)]

The segment tables (ix, fx, iy, fy, iz, fz) are taken as given, in fp32, exactly the values the kernel is handed; the
weights are formed from them in float64, where 1 - f and the products are exact to 2^-53.  Segment i of an axis of n
nodes has the nodes i and min(i + 1, n - 1).  render_volume_f64 is the definition; volume_grad_f64 its autograd gradient
in V; the *_abs variants are the same sums on magnitudes (the weights are not negative); sampled_out / sampled_dvol
evaluate single output pixels and single dV elements directly from the formulas above -- for sizes whose full float64
result is too slow -- and tests/test_render_volume_cpu.py holds them against the full restatement."""
import torch

from render_f64 import render_f64


def _axis(i, f, n, upper):
    """Node index and float64 weight of a segment table's lower or upper end."""
    i = i.long().clamp(0, max(n - 2, 0))
    return ((i + 1).clamp(max=n - 1), f.double()) if upper else (i, 1.0 - f.double())


def corners(tables, dims):
    """The 8 corners of every pixel: (zi [B,H,W], yi [1,H,1], xi [1,1,W], w [B,H,W] float64) each."""
    ix, fx, iy, fy, iz, fz = tables
    dz, gy, gx = dims
    for kz in (0, 1):
        zi, wz = _axis(iz, fz, dz, kz)
        for ky in (0, 1):
            yi, wy = _axis(iy, fy, gy, ky)
            for kx in (0, 1):
                xi, wx = _axis(ix, fx, gx, kx)
                yield zi, yi.reshape(1, -1, 1), xi.reshape(1, 1, -1), (wz * wy.reshape(1, -1, 1)) * wx.reshape(1, 1, -1)


def interpolate_kernels(vol, tables):
    """V [Dz,Gy,Gx,2,ks,ks] -> the per-pixel kernels [B,H,W,2,ks,ks] (torch ops: differentiable in V)."""
    out = 0
    for zi, yi, xi, w in corners(tables, vol.shape[:3]):
        out = out + w.to(vol.dtype)[..., None, None, None] * vol[zi, yi, xi]
    return out


def render_volume_f64(img, vol, tables, ks):
    """-> (left, right), each [B,C,H,W], in float64."""
    return render_f64(img.double(), interpolate_kernels(vol.double(), tables), ks)


def volume_grad_f64(img, vol_shape, tables, gl, gr, ks):
    """d/dV of (gl * left).sum() + (gr * right).sum() by autograd on render_volume_f64 (linear in V: V's value is
    irrelevant)."""
    vol = torch.zeros(vol_shape, dtype=torch.float64, device=img.device, requires_grad=True)
    left, right = render_volume_f64(img, vol, tables, ks)
    return torch.autograd.grad((gl.double() * left).sum() + (gr.double() * right).sum(), vol)[0]


def render_volume_abs(img, vol, tables, ks):
    """Per output element the sum of the magnitudes of its 8 ks^2 terms."""
    return render_volume_f64(img.abs(), vol.abs(), tables, ks)


def volume_grad_abs(img, vol_shape, tables, gl, gr, ks):
    """Per dV element the sum of the magnitudes of its terms."""
    return volume_grad_f64(img.abs(), vol_shape, tables, gl.abs(), gr.abs(), ks)


def node_pixel_counts(tables, dims):
    """[Dz,Gy,Gx]: how many (b, pixel) have a non-zero weight at each node (n of the gradient bar is C times that).
    A pixel whose segment has the node at both ends (an axis of one node) counts once."""
    dz, gy, gx = dims
    b, h, w = tables[4].shape
    touched = torch.zeros((b, h, w, dz * gy * gx), dtype=torch.bool, device=tables[4].device)
    for zi, yi, xi, wt in corners(tables, dims):
        flat = ((zi * gy + yi) * gx + xi)
        touched.scatter_(3, flat.unsqueeze(-1), (wt != 0).unsqueeze(-1) | touched.gather(3, flat.unsqueeze(-1)))
    return touched.sum((0, 1, 2)).reshape(dz, gy, gx)


def _node_weight(i, f, n, g):
    """float64 weight of node g in the segments (i, f) of an axis of n nodes."""
    lo, wlo = _axis(i, f, n, 0)
    hi, whi = _axis(i, f, n, 1)
    return wlo * (lo == g) + whi * (hi == g)


def sampled_out(img, vol, tables, ks, idx, absolute=False):
    """out_s[b,c,y,x] for both sides at the rows (b, c, y, x) of idx [S,4] -> [S,2]."""
    pad = (ks - 1) // 2
    _, _, h, w = img.shape
    ix, fx, iy, fy, iz, fz = tables
    dz, gy, gx = vol.shape[:3]
    b, c, y, x = idx.unbind(1)
    img, vol = img.double(), vol.double()
    if absolute:
        img, vol = img.abs(), vol.abs()
    K = 0
    for kz in (0, 1):
        zi, wz = _axis(iz[b, y, x], fz[b, y, x], dz, kz)
        for ky in (0, 1):
            yi, wy = _axis(iy[y], fy[y], gy, ky)
            for kx in (0, 1):
                xi, wx = _axis(ix[x], fx[x], gx, kx)
                K = K + ((wz * wy) * wx)[:, None, None, None] * vol[zi, yi, xi]            # [S,2,ks,ks]
    taps = torch.arange(ks, device=img.device)
    yy = (y[:, None] + pad - taps[None, :]).clamp(0, h - 1)                                # tap i reads row y + pad - i
    xx = (x[:, None] + pad - taps[None, :]).clamp(0, w - 1)
    patch = img[b[:, None, None], c[:, None, None], yy[:, :, None], xx[:, None, :]]        # [S,ks,ks]
    return (K * patch[:, None]).sum((-1, -2))


def sampled_dvol(img, gl, gr, tables, dims, ks, idx, absolute=False):
    """dV[dz,gy,gx,s,i,j] at the rows of idx [S,6] -> (values [S], pixels with a non-zero weight at the node [S])."""
    pad = (ks - 1) // 2
    bsz, ch, h, w = img.shape
    ix, fx, iy, fy, iz, fz = tables
    dz, gy, gx = dims
    G = torch.stack((gl, gr)).double()
    img = img.double()
    if absolute:
        G, img = G.abs(), img.abs()
    rows, cols = torch.arange(h, device=img.device), torch.arange(w, device=img.device)
    vals, counts = [], []
    for z_, y_, x_, s, i, j in idx.tolist():
        wt = (_node_weight(iz, fz, dz, z_) * _node_weight(iy, fy, gy, y_).reshape(1, -1, 1)) \
            * _node_weight(ix, fx, gx, x_).reshape(1, 1, -1)                               # [B,H,W]
        yy, xx = (rows + pad - i).clamp(0, h - 1), (cols + pad - j).clamp(0, w - 1)
        D = (G[s] * img[:, :, yy][:, :, :, xx]).sum(1)                                     # [B,H,W]
        vals.append((wt * D).sum())
        counts.append((wt != 0).sum())
    return torch.stack(vals), torch.stack(counts)
