"""Image-space per-pixel dual-pixel PSF convolution (consumer of the PSFs).

Same signatures as deeplens/render_psf.py:76-188.  The reference materialises
an unfold buffer [B, C*ks*ks, H*W] (1 GB at 512x768, ks 21) and multiplies it
with the per-pixel kernels; here one HIP kernel gathers the ks*ks neighbourhood
of every output pixel and reads each per-pixel kernel exactly once.
"""
import dataclasses

import torch

from . import _lib
from .basics import DEFAULT_WAVE, dptr, stream_ptr


def _render(input, psf, kernel_size, half):
    if input.dim() < 4:
        input = input.unsqueeze(0)
    if input.device.type != "cuda":
        raise _lib.SdirtError("sdirt_amd renders on the GPU only (no CPU fallback)")
    b, c, h, w = input.shape
    img = input.to(torch.float32).contiguous()
    k = psf.to(torch.float32).reshape(b, h, w, 2, kernel_size, kernel_size).contiguous()
    rl = torch.empty((b, c, h, w), dtype=torch.float32, device=input.device)
    rr = torch.empty_like(rl)
    _lib.check(_lib.lib().sdirt_local_psf_render(dptr(img), dptr(k), b, c, h, w, kernel_size,
                                                 1 if half else 0, dptr(rl), dptr(rr),
                                                 stream_ptr(input.device)))
    return rl.to(input.dtype), rr.to(input.dtype)


def local_psf_render(input, psf, kernel_size=11, val=False):
    """render_psf.py:76-118 (fp16 arithmetic) -> (rl, rr) [N,C,H,W]."""
    return _render(input, psf, kernel_size, half=True)


def local_psf_render_fast(input, psf, kernel_size=11, val=False):
    """render_psf.py:120-155 (fp16 arithmetic) -> (rl, rr) [N,C,H,W]."""
    return _render(input, psf, kernel_size, half=True)


def _grad_halves(grad, c):
    """The upstream gradient of cat(left, right) [B,2C,H,W] -> its two halves, fp32 and contiguous, as the kernels
    read them."""
    return grad[:, :c].to(torch.float32).contiguous(), grad[:, c:].to(torch.float32).contiguous()


class _LocalDpPsfRender(torch.autograd.Function):
    """local_dp_psf_render under autograd: the forward is _render's kernel call on the same operands (bit-equal to
    the no-grad call), the backward the two kernels of sdirt_render_grad.hip -- only those ctx.needs_input_grad asks
    for."""

    @staticmethod
    def forward(ctx, input, dp_psf, kernel_size):
        rl, rr = _render(input, dp_psf, kernel_size, half=False)
        ctx.save_for_backward(input, dp_psf)
        ctx.kernel_size = kernel_size
        return torch.cat([rl, rr], dim=1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        input, dp_psf = ctx.saved_tensors
        ks = ctx.kernel_size
        b, c, h, w = input.shape if input.dim() == 4 else (1, *input.shape)
        lib, stream = _lib.lib(), stream_ptr(input.device)
        gl, gr = _grad_halves(grad, c)
        grad_input = grad_psf = None
        if ctx.needs_input_grad[0]:
            k = dp_psf.to(torch.float32).reshape(b, h, w, 2, ks, ks).contiguous()
            nbytes = lib.sdirt_local_psf_render_grad_img_workspace_bytes(b, c, h, w, ks)
            if nbytes < 0:
                raise _lib.SdirtError(f"local_dp_psf_render has no backward for kernel_size={ks}")
            work = torch.empty(nbytes // 4, dtype=torch.float32, device=input.device)
            gi = torch.empty((b, c, h, w), dtype=torch.float32, device=input.device)
            _lib.check(lib.sdirt_local_psf_render_grad_img(dptr(k), dptr(gl), dptr(gr), b, c, h, w, ks, dptr(gi),
                                                           dptr(work), nbytes, stream))
            grad_input = gi.to(input.dtype).reshape(input.shape)
        if ctx.needs_input_grad[1]:
            img = input.to(torch.float32).contiguous()
            gk = torch.empty((b, h, w, 2, ks, ks), dtype=torch.float32, device=input.device)
            _lib.check(lib.sdirt_local_psf_render_grad_psf(dptr(img), dptr(gl), dptr(gr), b, c, h, w, ks, dptr(gk),
                                                           stream))
            grad_psf = gk.to(dp_psf.dtype).reshape(dp_psf.shape)
        return grad_input, grad_psf, None


def local_dp_psf_render(input, dp_psf, kernel_size=21):
    """render_psf.py:157-188 (fp32) -> [N, 2C, H, W] = cat(left, right).  Differentiable in `input` and `dp_psf`,
    as the reference's torch ops are: a call in grad mode on an operand that requires a gradient goes through
    _LocalDpPsfRender (same forward kernel, same values); every other call is the plain kernel call."""
    if torch.is_grad_enabled() and (input.requires_grad or dp_psf.requires_grad):
        return _LocalDpPsfRender.apply(input, dp_psf, kernel_size)
    rl, rr = _render(input, dp_psf, kernel_size, half=False)
    return torch.cat([rl, rr], dim=1)


def axis_segments(nodes, t):
    """Where the coordinates `t` (any shape) fall on a 1-D axis of strictly monotone `nodes` (increasing or
    decreasing), in fp32 -> (i int32, f fp32), each shaped like t: t lies between nodes[i] and nodes[i + 1], i clamped
    to [0, n - 2], and f = clamp((t - nodes[i]) / (nodes[i + 1] - nodes[i]), 0, 1) -- outside the node range the end
    node alone counts (constant extrapolation).  A t exactly on the last node gives (n - 2, 1).  An axis of one node
    gives i = 0, f = 0."""
    nodes = nodes.to(torch.float32).reshape(-1)
    t = t.to(device=nodes.device, dtype=torch.float32)
    n = nodes.numel()
    if n < 1:
        raise ValueError("axis_segments needs at least one node")
    if n == 1:
        return torch.zeros(t.shape, dtype=torch.int32, device=t.device), torch.zeros_like(t)
    ascending = bool(nodes[-1] > nodes[0])
    steps = nodes[1:] - nodes[:-1]
    if not bool(((steps > 0) if ascending else (steps < 0)).all()):
        raise ValueError("axis_segments needs strictly monotone nodes")
    # decreasing nodes: the same search on the negated axis (negation is exact)
    key, val = (nodes, t) if ascending else (-nodes, -t)
    i = (torch.searchsorted(key.contiguous(), val.contiguous(), right=True) - 1).clamp(0, n - 2)
    lo, hi = nodes[i], nodes[i + 1]
    f = ((t - lo) / (hi - lo)).clamp(0.0, 1.0) + 0.0                      # (+ 0.0: a -0 of a decreasing axis becomes 0)
    return i.to(torch.int32), f


def volume_segment_tables(x_nodes, y_nodes, z_nodes, z, height, width):
    """The six segment tables of local_dp_psf_render_volume for an image of height x width pixels and the normalised
    depth map z [B,H,W]: pixel x = linspace(-1, 1, W), pixel y = linspace(1, -1, H) (the render grid of
    psfnet.py:684-688) -> (ix [W], fx [W], iy [H], fy [H], iz [B,H,W], fz [B,H,W]) on z's device."""
    dev = z.device
    ix, fx = axis_segments(x_nodes.to(dev), torch.linspace(-1, 1, width, device=dev))
    iy, fy = axis_segments(y_nodes.to(dev), torch.linspace(1, -1, height, device=dev))
    iz, fz = axis_segments(z_nodes.to(dev), z)
    return tuple(t.contiguous() for t in (ix, fx, iy, fy, iz, fz))


def _volume_shape(img, volume, tables, ks):
    b, c, h, w = img.shape
    dz, gy, gx = volume.shape[-6:-3] if volume.dim() in (6, 7) else (0, 0, 0)
    if volume.dim() not in (6, 7) or tuple(volume.shape[-6:]) != (dz, gy, gx, 2, ks, ks):
        raise ValueError(f"volume must be [Dz, Gy, Gx, 2, {ks}, {ks}] or, chromatic, [C, Dz, Gy, Gx, 2, {ks}, {ks}], "
                         f"got {tuple(volume.shape)}")
    if volume.dim() == 7 and volume.shape[0] != c:
        raise ValueError(f"a chromatic volume holds one PSF volume per image channel: {volume.shape[0]} for an image of "
                         f"{c} channels")
    want = ((w,), (w,), (h,), (h,), (b, h, w), (b, h, w))
    for t, shape, dtype in zip(tables, want, (torch.int32, torch.float32) * 3):
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != img.device or not t.is_contiguous():
            raise ValueError(f"segment tables must be contiguous (int32, float32) pairs of shapes {want} on the image's device")
    return b, c, h, w, dz, gy, gx


def _volume_entry(volume_shape, suffix=""):
    """The C entry for a volume of this shape: sdirt_render_psf_volume<suffix>, or its _chroma sibling for a chromatic
    volume [C,Dz,Gy,Gx,2,ks,ks]."""
    return getattr(_lib.lib(), "sdirt_render_psf_volume" + ("_chroma" if len(volume_shape) == 7 else "") + suffix)


def _render_volume(img, volume, tables, ks):
    """img [B,C,H,W] and volume [Dz,Gy,Gx,2,ks,ks] or [C,Dz,Gy,Gx,2,ks,ks], fp32 contiguous on the GPU -> (left, right)
    [B,C,H,W]."""
    if img.device.type != "cuda":
        raise _lib.SdirtError("sdirt_amd renders on the GPU only (no CPU fallback)")
    b, c, h, w, dz, gy, gx = _volume_shape(img, volume, tables, ks)
    rl = torch.empty((b, c, h, w), dtype=torch.float32, device=img.device)
    rr = torch.empty_like(rl)
    _lib.check(_volume_entry(volume.shape)(dptr(img), dptr(volume), *(dptr(t) for t in tables), b, c, h, w, ks,
                                           dz, gy, gx, dptr(rl), dptr(rr), stream_ptr(img.device)))
    return rl, rr


class _RenderPsfVolume(torch.autograd.Function):
    """local_dp_psf_render_volume under autograd: the forward is _render_volume's kernel call on the same operands
    (bit-equal to the no-grad call), the backward sdirt_render_psf_volume_grad.  A chromatic
    volume [C,Dz,Gy,Gx,2,ks,ks] goes through the _chroma entries, forward and backward (_volume_entry)."""

    @staticmethod
    def forward(ctx, volume, img, ks, *tables):
        vol = volume.to(torch.float32).contiguous()
        rl, rr = _render_volume(img, vol, tables, ks)
        ctx.save_for_backward(img, *tables)
        ctx.kernel_size, ctx.volume_shape, ctx.volume_dtype = ks, vol.shape, volume.dtype
        return torch.cat([rl, rr], dim=1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        img, *tables = ctx.saved_tensors
        b, c, h, w = img.shape
        dz, gy, gx = ctx.volume_shape[-6:-3]
        gl, gr = _grad_halves(grad, c)
        dvol = torch.empty(ctx.volume_shape, dtype=torch.float32, device=img.device)
        _lib.check(_volume_entry(ctx.volume_shape, "_grad")(dptr(img), dptr(gl), dptr(gr), *(dptr(t) for t in tables),
                                                            b, c, h, w, ctx.kernel_size, dz, gy, gx, dptr(dvol),
                                                            stream_ptr(img.device)))
        return (dvol.to(ctx.volume_dtype), None, None) + (None,) * len(tables)


class _RenderPsfVolumeScene(torch.autograd.Function):
    """local_dp_psf_render_volume(..., scene_grad=True) under autograd: the forward is _render_volume's kernel call on
    the same operands (bit-equal to the plain call); the backward calls only what ctx.needs_input_grad asks for --
    sdirt_render_psf_volume_grad for the volume, sdirt_render_psf_volume_grad_scene for the image, the depth table
    value fz or both, with NULL for the one that is not wanted.  The step from fz to z is
    axis_segments' torch ops, outside this Function.  A chromatic volume goes through the _chroma entries."""

    @staticmethod
    def forward(ctx, volume, img, fz, ks, ix, fx, iy, fy, iz):
        vol = volume.to(torch.float32).contiguous()
        rl, rr = _render_volume(img, vol, (ix, fx, iy, fy, iz, fz), ks)
        ctx.save_for_backward(vol, img, fz, ix, fx, iy, fy, iz)
        ctx.kernel_size, ctx.volume_dtype = ks, volume.dtype
        return torch.cat([rl, rr], dim=1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        vol, img, fz, ix, fx, iy, fy, iz = ctx.saved_tensors
        tables = (ix, fx, iy, fy, iz, fz)
        b, c, h, w = img.shape
        dz, gy, gx = vol.shape[-6:-3]
        shape = (b, c, h, w, ctx.kernel_size, dz, gy, gx)
        stream = stream_ptr(img.device)
        gl, gr = _grad_halves(grad, c)
        dvol = dimg = dfz = None
        if ctx.needs_input_grad[0]:
            dvol = torch.empty(vol.shape, dtype=torch.float32, device=img.device)
            _lib.check(_volume_entry(vol.shape, "_grad")(dptr(img), dptr(gl), dptr(gr), *(dptr(t) for t in tables),
                                                         *shape, dptr(dvol), stream))
            dvol = dvol.to(ctx.volume_dtype)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            if ctx.needs_input_grad[1]:
                dimg = torch.empty(img.shape, dtype=torch.float32, device=img.device)
            if ctx.needs_input_grad[2]:
                dfz = torch.empty(fz.shape, dtype=torch.float32, device=img.device)
            _lib.check(_volume_entry(vol.shape, "_grad_scene")(dptr(img), dptr(vol), dptr(gl), dptr(gr),
                                                               *(dptr(t) for t in tables), *shape, dptr(dimg),
                                                               dptr(dfz), stream))
        return dvol, dimg, dfz, None, None, None, None, None, None


def local_dp_psf_render_volume(input, volume, x_nodes, y_nodes, z_nodes, z, kernel_size=21, scene_grad=False):
    """An image and its normalised depth map rendered into a dual-pixel pair straight from a PSF volume:
    local_dp_psf_render (render_psf.py:157-188) with the kernel of every pixel interpolated trilinearly in (x, y, z)
    from the eight grid PSFs around it, inside the HIP kernel -- the [B,H,W,2,ks,ks] tensor never exists.
    -> [B, 2C, H, W] = cat(left, right).

    input [B,C,H,W]; volume [Dz,Gy,Gx,2,ks,ks] (z-major, then rows, then columns: the order of a VolumeStepper block);
    x_nodes [Gx], y_nodes [Gy], z_nodes [Dz] strictly monotone (axis_segments); z [B,H,W] in the units of z_nodes.
    Pixel x = linspace(-1, 1, W), pixel y = linspace(1, -1, H).  Outside the nodes the end PSF is used.  The kernel
    does no normalisation: sum-normalised node PSFs give sum-normalised per-pixel kernels.

    A CHROMATIC volume [C,Dz,Gy,Gx,2,ks,ks] (Lensgroup.psf_volume with a sequence of wavelengths) renders channel c of
    the image with volume[c], in the same single kernel call; its leading extent must be the image's C (ValueError
    otherwise).  Everything below holds for it unchanged, the gradients included.

    Differentiable in `volume` (a call in grad mode on a volume that requires a gradient goes through _RenderPsfVolume:
    same forward kernel, same values).  By default gradients in the image and in the depth are not taken: asking for
    them raises.

    scene_grad=True opts in to them: a call in grad mode with `input`, `z` or `volume` requiring a gradient goes through
    _RenderPsfVolumeScene (same forward kernel, same values) and is differentiable in all three.  The kernel gives the
    gradient in the table value fz; from there to z it is axis_segments' torch ops, so torch's rules hold at the kinks:
    slope 1 / (nodes[i+1] - nodes[i]) of the segment the table names, also for a z exactly on a node, and exactly 0
    outside the node range.  `input.grad` comes back in the input's dtype.  Under no_grad, or with nothing requiring a
    gradient, scene_grad=True is the plain call."""
    if input.dim() < 4:
        input = input.unsqueeze(0)
    if volume.dim() == 7 and volume.shape[0] != input.shape[1]:
        raise ValueError(f"local_dp_psf_render_volume: a chromatic volume holds one PSF volume per image channel, got "
                         f"{volume.shape[0]} for an image of {input.shape[1]} channels")
    grad_mode = torch.is_grad_enabled()
    if scene_grad and grad_mode and (input.requires_grad or z.requires_grad or volume.requires_grad):
        b, _, h, w = input.shape
        img = input.to(torch.float32).contiguous()
        # volume_segment_tables on a z that is NOT detached: the plain call's table values, fz differentiable in z
        zz = z.to(img.device).reshape(b, h, w)
        ix, fx, iy, fy, iz, fz = volume_segment_tables(x_nodes.detach(), y_nodes.detach(), z_nodes.detach(), zz, h, w)
        if zz.requires_grad and not fz.requires_grad:
            fz = (fz + 0.0 * zz.to(torch.float32)).contiguous()  # an axis of one node: fz = 0 for every z, z.grad = 0
        out = _RenderPsfVolumeScene.apply(volume.to(img.device), img, fz, kernel_size, ix, fx, iy, fy, iz)
        return out.to(input.dtype)
    if grad_mode and input.requires_grad:
        raise ValueError("local_dp_psf_render_volume: the gradient with respect to the image is not built "
                         "(detach the image; local_dp_psf_render has one)")
    if grad_mode and z.requires_grad:
        raise ValueError("local_dp_psf_render_volume: the gradient with respect to the depth is not built (detach z)")
    b, _, h, w = input.shape
    img = input.detach().to(torch.float32).contiguous()
    zz = z.detach().to(img.device).reshape(b, h, w)
    tables = volume_segment_tables(x_nodes.detach(), y_nodes.detach(), z_nodes.detach(), zz, h, w)
    volume = volume.to(img.device)
    if grad_mode and volume.requires_grad:
        return _RenderPsfVolume.apply(volume, img, kernel_size, *tables).to(input.dtype)
    rl, rr = _render_volume(img, volume.detach().to(torch.float32).contiguous(), tables, kernel_size)
    return torch.cat([rl, rr], dim=1).to(input.dtype)


def photometric_scale(psf, energy):
    """Sum-normalised node PSFs -> PSFs that carry their energy: psf [..., 2, ks, ks] (a PSFVolume's psf, or any batch
    of (left, right) pairs) times energy[..., side] / mean(energy[..., :2]), energy [..., 3] = (E_L, E_R, T) of
    Lensgroup.psf_lr(energy=True) with the same leading shape.  The mean runs over all nodes and both sides, so the
    kernel sums of a scaled volume average 1: the definition is free of a gain (exposure is a scalar of any fit) and
    keeps what the data can show -- vignetting across the field and the left / right shading.  A chromatic volume
    [C, Dz, Gy, Gx, 2, ks, ks] with energy [C, Dz, Gy, Gx, 3] is scaled wavelength by wavelength, each by its own mean.
    torch ops throughout: differentiable in psf and in energy.  The render kernels normalise nothing, so a scaled
    volume renders shading as it stands."""
    if energy.shape[-1] != 3 or tuple(energy.shape[:-1]) != tuple(psf.shape[:-3]) or psf.shape[-3] != 2:
        raise ValueError(f"photometric_scale: psf [..., 2, ks, ks] and energy [..., 3] must share their leading shape, "
                         f"got {tuple(psf.shape)} and {tuple(energy.shape)}")
    e = energy[..., :2].to(device=psf.device, dtype=torch.float64)
    waves = e.shape[0] if psf.dim() == 7 else 1
    mean = e.reshape(waves, -1).mean(1).reshape((waves,) + (1,) * (e.dim() - 1) if psf.dim() == 7 else ())
    return psf * (e / mean).to(psf.dtype).unsqueeze(-1).unsqueeze(-1)


@dataclasses.dataclass
class PSFVolume:
    """A ray-traced PSF grid as local_dp_psf_render_volume consumes it (Lensgroup.psf_volume makes one).
    psf [Dz,Gy,Gx,2,ks,ks]: left and right PSF of every node, each sum-normalised; x_nodes [Gx], y_nodes [Gy]:
    normalised sensor coordinates (y decreases, as the image's rows do); z_nodes [Dz]: normalised depth
    z = (depth - d_min) / (d_max - d_min) (PSFNet.depth2z), depth in mm.  wvln: the wavelengths (um) the PSFs were
    traced at -- one: psf is the 6-D volume above; several: psf is chromatic, [len(wvln),Dz,Gy,Gx,2,ks,ks], psf[c] the
    volume of wvln[c], rendered into channel c.  energy: None, or -- psf_volume(photometric=True) -- the nodes'
    (E_L, E_R, T) [Dz,Gy,Gx,3] ([len(wvln),Dz,Gy,Gx,3]) the PSFs were scaled with (photometric_scale): their sums are
    then energy / mean(energy) instead of 1.  It is the trailing argument of the constructor and an attribute of the
    volume (dataclasses.replace carries it over), declared init-only so that dataclasses.fields() -- the tensors a
    volume is made of, ending with wvln -- stays what it was."""
    psf: torch.Tensor
    x_nodes: torch.Tensor
    y_nodes: torch.Tensor
    z_nodes: torch.Tensor
    d_min: float
    d_max: float
    wvln: tuple = (DEFAULT_WAVE,)
    energy: dataclasses.InitVar[torch.Tensor] = None

    def __post_init__(self, energy):
        self.energy = energy

    def points(self):
        """[Dz*Gy*Gx, 3] points (x, y normalised, depth in mm) in the volume's order: what psf_lr is given."""
        depth = self.z_nodes.to(torch.float32) * (self.d_max - self.d_min) + self.d_min
        dz, gy, gx = len(self.z_nodes), len(self.y_nodes), len(self.x_nodes)
        x = self.x_nodes.to(torch.float32).reshape(1, 1, gx).expand(dz, gy, gx)
        y = self.y_nodes.to(torch.float32).reshape(1, gy, 1).expand(dz, gy, gx)
        return torch.stack((x, y, depth.reshape(dz, 1, 1).expand(dz, gy, gx)), -1).reshape(-1, 3).contiguous()

    def render(self, input, z, scene_grad=False):
        """local_dp_psf_render_volume of this volume (scene_grad=True: differentiable in `input` and `z` as well)."""
        return local_dp_psf_render_volume(input, self.psf, self.x_nodes, self.y_nodes, self.z_nodes, z,
                                          self.psf.shape[-1], scene_grad=scene_grad)


def psfnet_render(input, raw_l, raw_r, kernel_size):
    """PSFNet.pred + local_psf_render_fast (psfnet.py:317-336, 702-707; render_psf.py:120-155)
    in one pass over the network's raw fp16 outputs raw_l = net(x, y, z), raw_r = net(-x, y, z),
    each [B,H,W,ks,ks]: the stacked, flipped, normalised per-pixel kernels are formed in LDS
    only.  -> (rl, rr) [B,C,H,W] fp32 holding fp16 values, as local_psf_render_fast returns."""
    if input.device.type != "cuda":
        raise _lib.SdirtError("sdirt_amd renders on the GPU only (no CPU fallback)")
    b, c, h, w = input.shape
    img = input.to(torch.float32).contiguous()
    raw_l = raw_l.to(torch.float16).reshape(b, h, w, kernel_size * kernel_size).contiguous()
    raw_r = raw_r.to(torch.float16).reshape(b, h, w, kernel_size * kernel_size).contiguous()
    if raw_l.data_ptr() % 16:                  # the kernel stages with 16-byte loads
        raw_l = raw_l.clone()
    if raw_r.data_ptr() % 16:
        raw_r = raw_r.clone()
    rl = torch.empty((b, c, h, w), dtype=torch.float32, device=input.device)
    rr = torch.empty_like(rl)
    _lib.check(_lib.lib().sdirt_psfnet_render(dptr(img), dptr(raw_l), dptr(raw_r), b, c, h, w,
                                              kernel_size, dptr(rl), dptr(rr),
                                              stream_ptr(input.device)))
    return rl, rr


def local_psf_render_high_res(input, psf, patch_size=[320, 480], kernel_size=11):
    """render_psf.py:191-208: the image cut into patch_size tiles, every tile rendered on its own
    by local_psf_render -- so each tile is replicate-padded at ITS OWN border.  Returns (rl, rr)
    [N,C,H,W].  (The reference's version assigns local_psf_render's (left, right) tuple into one
    tensor and raises TypeError; this is what its loop computes with both halves kept, pinned by
    fixture F18 = the reference's local_psf_render applied tile by tile.)"""
    _, _, height, width = input.shape
    rl, rr = torch.zeros_like(input), torch.zeros_like(input)
    for top in range(0, height, patch_size[0]):
        for left in range(0, width, patch_size[1]):
            rows = slice(top, min(top + patch_size[0], height))
            cols = slice(left, min(left + patch_size[1], width))
            rl[:, :, rows, cols], rr[:, :, rows, cols] = local_psf_render(
                input[:, :, rows, cols], psf[:, rows, cols], kernel_size=kernel_size)
    return rl, rr


def _depthwise_convolution(padded, kernels):
    """True (flipped-kernel) 2-D convolution of every channel with its own [ks, ks] kernel, no
    further padding: stock depthwise conv2d (MIOpen), which correlates, on the flipped kernels."""
    flipped = kernels.flip(-2, -1).unsqueeze(1)                     # [C, 1, ks, ks]
    return torch.nn.functional.conv2d(padded, flipped, groups=padded.shape[1])


def render_psf(img, psf):
    """render_psf.py:12-28: one PSF per channel for the whole image, [B,C,H,W] * [C,ks,ks], reflect
    padding.  Dense depthwise convolution: library work, no custom kernel."""
    half = psf.shape[-1] // 2
    return _depthwise_convolution(torch.nn.functional.pad(img, (half,) * 4, mode="reflect"), psf)


def render_psf_map(img, psf_map, grid):
    """render_psf.py:31-73: psf_map [C, grid*ks, grid*ks] holds one PSF per image tile (tile (i, j)
    covers rows int(i/grid*H) .. int((i+1)/grid*H) and the matching columns); every tile is
    convolved with its PSF, reading across the tile border into the (reflect-padded) image."""
    assert img.dim() == 4, "Input image should be [B, C, H, W]"
    channels, map_h, map_w = psf_map.shape
    assert map_h % grid == 0 and map_w % grid == 0, "PSF map size should be divisible by grid"
    ks = map_h // grid
    assert ks % 2 == 1, "PSF kernel size should be odd"
    _, c, height, width = img.shape
    assert c == channels, "PSF map should have the same channel as image"
    half = (ks - 1) // 2
    padded = torch.nn.functional.pad(img, (half,) * 4, mode="reflect")
    tiles = psf_map.view(channels, grid, ks, grid, ks).permute(1, 3, 0, 2, 4)    # [grid, grid, C, ks, ks]
    row_edge = [int(i / grid * height) for i in range(grid + 1)]
    col_edge = [int(j / grid * width) for j in range(grid + 1)]
    out = torch.zeros_like(img)
    for i in range(grid):
        for j in range(grid):
            window = padded[:, :, row_edge[i]:row_edge[i + 1] + 2 * half, col_edge[j]:col_edge[j + 1] + 2 * half]
            out[:, :, row_edge[i]:row_edge[i + 1], col_edge[j]:col_edge[j + 1]] = \
                _depthwise_convolution(window, tiles[i, j])
    return out
