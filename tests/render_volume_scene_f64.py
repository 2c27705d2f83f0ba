"""The gradients of the render from a PSF volume with respect to the scene -- the image and the depth table value fz --
restated in torch (float64), for the tests of k_render_psf_volume_grad_img / _grad_depth.  Not a test file.

    dImg[b,c,v,u] = sum_s sum_{(y,x,i,j): clamp(y+pad-i) = v, clamp(x+pad-j) = u} G_s[b,c,y,x] * K_s(b,y,x)[i,j]
    dfz[b,y,x]    = sum_s sum_c G_s[b,c,y,x] * sum_{i,j} (dK_s/dfz)[i,j] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)]
    dK_s/dfz      = sum over the 8 corners of +-(wy * wx) * V[corner]        (+ upper depth plane, - lower)

scene_grads_f64 is torch autograd through the restatement of the forward (render_volume_f64.interpolate_kernels, whose
weights are 1 - f.double() and f.double(), then render_f64) in img.double() and in a float64 leaf that holds the fp32 fz
values: the specification.  The *_abs functions are the same sums on magnitudes, term by term.  sampled_dimg /
sampled_dfz evaluate single elements directly from the formulas above -- for sizes whose full float64 gradient is too
slow -- and tests/test_render_volume_scene_cpu.py holds them against the full restatement."""
import torch

from render_f64 import render_f64
from render_volume_f64 import _axis, interpolate_kernels


def scene_grads_f64(img, vol, tables, gl, gr, ks):
    """(d/d img [B,C,H,W], d/d fz [B,H,W]) of (gl * left).sum() + (gr * right).sum(), float64."""
    ix, fx, iy, fy, iz, fz = tables
    img = img.double().detach().requires_grad_(True)
    fz = fz.double().detach().requires_grad_(True)
    left, right = render_f64(img, interpolate_kernels(vol.double().detach(), (ix, fx, iy, fy, iz, fz)), ks)
    return torch.autograd.grad((gl.double() * left).sum() + (gr.double() * right).sum(), [img, fz])


def dimg_abs(img, vol, tables, gl, gr, ks):
    """Per dImg element the sum of the magnitudes of its terms (the weights are not negative)."""
    return scene_grads_f64(img.abs(), vol.abs(), tables, gl.abs(), gr.abs(), ks)[0]


def dfz_abs(img, vol, tables, gl, gr, ks):
    """Per dfz element the sum of the magnitudes of its terms: both depth planes count with +(wy * wx), which is the
    kernel at fz = 1 plus the kernel at fz = 0."""
    ix, fx, iy, fy, iz, fz = tables
    total = 0
    for value in (1.0, 0.0):
        k = interpolate_kernels(vol.double().abs(), (ix, fx, iy, fy, iz, torch.full_like(fz, value)))
        left, right = render_f64(img.double().abs(), k, ks)
        total = total + (gl.double().abs() * left).sum(1) + (gr.double().abs() * right).sum(1)
    return total


def fold_counts(h, w, ks):
    """[H,W]: how many padded positions clamp onto each image position (m of the dImg bar): 1 inside, pad + 1 on an
    edge, (pad + 1)^2 at a corner, 2 pad + 1 along an image of one row or column."""
    pad = (ks - 1) // 2
    one = lambda n: 1 + pad * ((torch.arange(n) == 0).long() + (torch.arange(n) == n - 1).long())
    return one(h)[:, None] * one(w)[None, :]


def sampled_dimg(vol, gl, gr, tables, ks, idx, absolute=False):
    """dImg[b,c,v,u] at the rows of idx [S,4] -> values [S]."""
    pad = (ks - 1) // 2
    _, _, h, w = gl.shape
    ix, fx, iy, fy, iz, fz = tables
    dz, gy, gx = vol.shape[:3]
    vol = vol.double().abs() if absolute else vol.double()
    taps = torch.arange(ks, device=vol.device)
    vals = []
    for b, c, v, u in idx.tolist():
        # the padded positions that clamp to (v, u); tap i of pixel y reads padded row y + pad - i: y = vp - pad + i
        vp = torch.arange(-pad if v == 0 else v, (h - 1 + pad if v == h - 1 else v) + 1, device=vol.device)
        up = torch.arange(-pad if u == 0 else u, (w - 1 + pad if u == w - 1 else u) + 1, device=vol.device)
        y = (vp[:, None] - pad + taps[None, :]).reshape(-1, 1)              # [nv * ks, 1]
        x = (up[:, None] - pad + taps[None, :]).reshape(1, -1)              # [1, nu * ks]
        i, j = taps.repeat(len(vp)).reshape(-1, 1), taps.repeat(len(up)).reshape(1, -1)
        ok = ((y >= 0) & (y < h)) & ((x >= 0) & (x < w))
        yc, xc = y.clamp(0, h - 1), x.clamp(0, w - 1)
        K = 0                                                               # [2, nv * ks, nu * ks]
        for kz in (0, 1):
            zi, wz = _axis(iz[b][yc, xc], fz[b][yc, xc], dz, kz)
            for ky in (0, 1):
                yi, wy = _axis(iy[yc], fy[yc], gy, ky)
                for kx in (0, 1):
                    xi, wx = _axis(ix[xc], fx[xc], gx, kx)
                    K = K + ((wz * wy) * wx) * torch.stack([vol[zi, yi, xi, s, i, j] for s in (0, 1)])
        G = torch.stack((gl[b, c][yc, xc], gr[b, c][yc, xc])).double()
        vals.append(((G.abs() if absolute else G) * K * ok).sum())
    return torch.stack(vals)


def sampled_dfz(img, vol, gl, gr, tables, ks, idx, absolute=False):
    """dfz[b,y,x] at the rows of idx [S,3] -> values [S]."""
    pad = (ks - 1) // 2
    _, _, h, w = img.shape
    ix, fx, iy, fy, iz, fz = tables
    dz, gy, gx = vol.shape[:3]
    b, y, x = idx.unbind(1)
    img, vol, G = img.double(), vol.double(), torch.stack((gl, gr)).double()
    if absolute:
        img, vol, G = img.abs(), vol.abs(), G.abs()
    dK = 0                                                                  # [S,2,ks,ks]
    (lower, _), (upper, _) = (_axis(iz[b, y, x], fz[b, y, x], dz, kz) for kz in (0, 1))
    for ky in (0, 1):
        yi, wy = _axis(iy[y], fy[y], gy, ky)
        for kx in (0, 1):
            xi, wx = _axis(ix[x], fx[x], gx, kx)
            # upper plane minus lower, pair by pair: exactly 0 where the two planes are the same node
            pair = vol[upper, yi, xi] + vol[lower, yi, xi] if absolute else vol[upper, yi, xi] - vol[lower, yi, xi]
            dK = dK + (wy * wx)[:, None, None, None] * pair
    taps = torch.arange(ks, device=img.device)
    yy = (y[:, None] + pad - taps[None, :]).clamp(0, h - 1)
    xx = (x[:, None] + pad - taps[None, :]).clamp(0, w - 1)
    patch = img[b[:, None, None], :, yy[:, :, None], xx[:, None, :]]        # [S,ks,ks,C]
    up = G[:, b, :, y, x]                                                   # [S,2,C]: the indexed dimensions lead
    D = (up[:, :, None, None, :] * patch[:, None]).sum(-1)                  # [S,2,ks,ks]
    return (dK * D).sum((1, 2, 3))
