"""The render of a dual-pixel pair from a CHROMATIC PSF volume [C,Dz,Gy,Gx,2,ks,ks] restated in torch (float64), for
the tests of the k_*_chroma kernels of sdirt_render_volume.hip.  Not a test file.

Channel c of the image is rendered with the volume V[c]; the segment tables, and so the weights, are shared:

    out_s[:, c]  = render_volume_f64(img[:, c:c+1], V[c])                      (tests/render_volume_f64.py)
    dV[c]        = volume_grad_f64(img[:, c:c+1], ..., G_l[:, c:c+1], G_r[:, c:c+1])    -- no sum over the channels
    dImg[:, c]   = scene_grads_f64(img[:, c:c+1], V[c], ...)[0]                (tests/render_volume_scene_f64.py)
    dfz          = sum_c scene_grads_f64(img[:, c:c+1], V[c], ...)[1]          summed in float64

Everything here is the achromatic restatement applied per channel and concatenated; the *_abs variants are the same
sums on magnitudes.  tests/test_render_volume_chroma_cpu.py holds it against the reference's local_dp_psf_render."""
import torch

from render_volume_f64 import render_volume_abs, render_volume_f64, volume_grad_abs, volume_grad_f64
from render_volume_scene_f64 import dfz_abs, dimg_abs, scene_grads_f64


def _channel(t, c):
    return t[:, c:c + 1]


def _render(one, img, vol, tables, ks):
    sides = [one(_channel(img, c), vol[c], tables, ks) for c in range(img.shape[1])]
    return torch.cat([s[0] for s in sides], 1), torch.cat([s[1] for s in sides], 1)


def render_volume_chroma_f64(img, vol, tables, ks):
    """-> (left, right), each [B,C,H,W], in float64."""
    return _render(render_volume_f64, img, vol, tables, ks)


def render_volume_chroma_abs(img, vol, tables, ks):
    """Per output element the sum of the magnitudes of its 8 ks^2 terms."""
    return _render(render_volume_abs, img, vol, tables, ks)


def _volume_grad(one, img, vol_shape, tables, gl, gr, ks):
    return torch.stack([one(_channel(img, c), vol_shape[1:], tables, _channel(gl, c), _channel(gr, c), ks)
                        for c in range(img.shape[1])])


def volume_grad_chroma_f64(img, vol_shape, tables, gl, gr, ks):
    """d/dV [C,Dz,Gy,Gx,2,ks,ks] of (gl * left).sum() + (gr * right).sum()."""
    return _volume_grad(volume_grad_f64, img, vol_shape, tables, gl, gr, ks)


def volume_grad_chroma_abs(img, vol_shape, tables, gl, gr, ks):
    """Per dV element the sum of the magnitudes of its terms."""
    return _volume_grad(volume_grad_abs, img, vol_shape, tables, gl, gr, ks)


def scene_grads_chroma_f64(img, vol, tables, gl, gr, ks):
    """(d/d img [B,C,H,W], d/d fz [B,H,W]) of (gl * left).sum() + (gr * right).sum(), float64."""
    per = [scene_grads_f64(_channel(img, c), vol[c], tables, _channel(gl, c), _channel(gr, c), ks)
           for c in range(img.shape[1])]
    return torch.cat([p[0] for p in per], 1), torch.stack([p[1] for p in per]).sum(0)


def dimg_chroma_abs(img, vol, tables, gl, gr, ks):
    """Per dImg element the sum of the magnitudes of its terms."""
    return torch.cat([dimg_abs(_channel(img, c), vol[c], tables, _channel(gl, c), _channel(gr, c), ks)
                      for c in range(img.shape[1])], 1)


def dfz_chroma_abs(img, vol, tables, gl, gr, ks):
    """Per dfz element the sum of the magnitudes of its terms, all channels."""
    return torch.stack([dfz_abs(_channel(img, c), vol[c], tables, _channel(gl, c), _channel(gr, c), ks)
                        for c in range(img.shape[1])]).sum(0)
