"""The per-pixel dual-pixel PSF convolution restated in torch (float64 on the CPU by default), for the tests of its
backward kernels.  Not a test file.

    P = replicate_pad(img, (ks - 1) / 2)
    out_s[b,c,y,x] = sum_{i,j} K[b,y,x,s,i,j] * P[b,c, y + ks-1-i, x + ks-1-j]          s in {left, right}

Tap (i, j) of the stored kernel multiplies the neighbour at the FLIPPED offset.  render_f64 is that sum, tap by tap; its
gradients come from torch autograd (grads_f64).  sampled_grad_psf / sampled_grad_img evaluate the two gradient formulas
directly at chosen elements -- for sizes whose full gradient does not fit -- and tests/test_render_grad_cpu.py holds
them against the autograd ones."""
import torch
import torch.nn.functional as F


def render_f64(img, psf, ks):
    """img [B,C,H,W], psf [B,H,W,2,ks,ks] (any shape that reshapes to it) -> (left, right), each [B,C,H,W]."""
    b, c, h, w = img.shape
    pad = (ks - 1) // 2
    P = F.pad(img, (pad, pad, pad, pad), mode="replicate")
    K = psf.reshape(b, h, w, 2, ks, ks).permute(3, 0, 1, 2, 4, 5).unsqueeze(2)     # [2,B,1,H,W,ks,ks]
    out = torch.zeros((2, b, c, h, w), dtype=img.dtype, device=img.device)
    for i in range(ks):
        for j in range(ks):
            out = out + K[..., i, j] * P[:, :, ks - 1 - i:ks - 1 - i + h, ks - 1 - j:ks - 1 - j + w]
    return out[0], out[1]


def grads_f64(img, psf, gl, gr, ks):
    """(d/d img, d/d psf) of (gl * left).sum() + (gr * right).sum(), by autograd on render_f64 in float64."""
    img = img.double().detach().requires_grad_(True)
    psf = psf.double().detach().requires_grad_(True)
    left, right = render_f64(img, psf, ks)
    return torch.autograd.grad((gl.double() * left).sum() + (gr.double() * right).sum(), [img, psf])


def abs_terms_f64(img, psf, gl, gr, ks):
    """Per gradient element the sum of the magnitudes of its terms, (for d img, for d psf): the same sums on the
    operands' absolute values, where every term is its own magnitude."""
    return grads_f64(img.abs(), psf.abs(), gl.abs(), gr.abs(), ks)


def term_counts(shape, ks):
    """How many terms the sum of each d img element has ([B,C,H,W]; 2 ks^2 inside a large image, more on the
    borders, fewer where the image ends inside the window); every d psf element has C."""
    b, c, h, w = shape
    one = torch.ones(shape, dtype=torch.float64)
    return grads_f64(one, torch.ones((b, h, w, 2, ks, ks), dtype=torch.float64), one, one, ks)[0]


def sampled_grad_psf(img, gl, gr, ks, idx, absolute=False):
    """d psf[b,y,x,s,i,j] = sum_c G_s[b,c,y,x] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)] at the rows of idx [S,6]."""
    pad = (ks - 1) // 2
    _, _, h, w = img.shape
    b, y, x, s, i, j = idx.unbind(1)
    G = torch.stack((gl, gr)).double()
    img = img.double()
    if absolute:
        G, img = G.abs(), img.abs()
    yy, xx = (y + pad - i).clamp(0, h - 1), (x + pad - j).clamp(0, w - 1)
    return (G[s, b, :, y, x] * img[b, :, yy, xx]).sum(1)


def sampled_grad_img(psf, gl, gr, ks, idx, absolute=False):
    """d img[b,c,v,u] = sum_s sum_{(y,x,i,j): clamp(y+pad-i) = v, clamp(x+pad-j) = u} G_s[b,c,y,x] K[b,y,x,s,i,j] at
    the rows of idx [S,4] -> (values [S], number of terms [S])."""
    pad = (ks - 1) // 2
    _, _, h, w = gl.shape
    K = psf.reshape(gl.shape[0], h, w, 2, ks, ks)
    taps = torch.arange(ks, device=psf.device)
    vals, counts = [], []
    for b, c, v, u in idx.tolist():
        # the padded positions that clamp to (v, u)
        vp = torch.arange(-pad if v == 0 else v, (h - 1 + pad if v == h - 1 else v) + 1, device=psf.device)
        up = torch.arange(-pad if u == 0 else u, (w - 1 + pad if u == w - 1 else u) + 1, device=psf.device)
        # tap i of pixel y reads padded row y + pad - i: y = vp - pad + i
        y = (vp[:, None] - pad + taps[None, :]).reshape(-1, 1)             # [nv * ks, 1]
        x = (up[:, None] - pad + taps[None, :]).reshape(1, -1)             # [1, nu * ks]
        i, j = taps.repeat(len(vp)).reshape(-1, 1), taps.repeat(len(up)).reshape(1, -1)
        ok = ((y >= 0) & (y < h)) & ((x >= 0) & (x < w))
        yc, xc = y.clamp(0, h - 1), x.clamp(0, w - 1)
        total = 0.0
        for s, g in enumerate((gl, gr)):
            t = g[b, c][yc, xc].double() * K[b][yc, xc, s, i, j].double()
            t = t.abs() if absolute else t
            total = total + (t * ok).sum()
        vals.append(total)
        counts.append(2 * int(ok.sum()))
    return torch.stack(vals), torch.tensor(counts)
