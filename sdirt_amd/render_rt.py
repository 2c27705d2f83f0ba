"""Ray-traced dual-pixel rendering of a textured plane through the lens: the backward renderer the
reference names in render_single_img(method='raytracing') (deeplens/optics.py:756-780) and never defines.

The reference has the ray generator (sample_sensor, optics.py:497-538), the trace to object space (trace2obj,
:630-635) and the caller; `render_sample_ray` and `render_compute_image` do not exist there.  Here the whole per-ray
program -- sample a sensor-side ray, take its dual-pixel weights from the direction it arrives with, trace it backward
through every surface, carry it to the plane, read the texture, sum -- is ONE HIP kernel (sdirt_render_plane,
csrc/sdirt_render_rt.hip); this module is its host side, the reference's two samplers, `render_single_img`, and a
pure-torch float64 restatement of the lookup and the sums (`plane_sums_float64`) that tests and tools check it with.

The layered render (render_layers, render_rgbd) and the opt-in gradients of all three renders in the
textures and the coverage (scene_grad=True, sdirt_render_layers_grad), in the dual-pixel parameters
h, f, w (dp_grad=True, sdirt_render_layers_dp_grad) and in the layer depths and scales (depth_grad=True,
sdirt_render_layers_depth_grad) live here as well.

Functions take the lens as their first argument; Lensgroup binds them under the reference's method names.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .basics import DEFAULT_WAVE, DEPTH, WAVE_RGB, Ray, dptr, stream_ptr

#: samples per pixel of one kernel launch, and so of one batch of the Newton trip rule (optics.py:769-776 renders a
#: high-spp image in rounds of 64)
CHUNK_SPP = 64


# ------------------------------------------------------------------------------------ the reference's samplers
def sensor_axes(lens, pixel_center=False):
    """(x1 [W], y1 [H]) fp32 on the lens's device: the sensor coordinates sample_sensor starts its rays from
    (optics.py:510-515: the bottom-right corner of every pixel), or with pixel_center the pixel centres
    x1 - ps / 2, y1 + ps / 2 (evaluated in fp32)."""
    H, W = lens.sensor_res
    x1 = torch.linspace(-lens.sensor_size[1] / 2, lens.sensor_size[1] / 2, W + 1, device=lens.device)[1:]
    y1 = torch.linspace(lens.sensor_size[0] / 2, -lens.sensor_size[0] / 2, H + 1, device=lens.device)[1:]
    if pixel_center:
        x1, y1 = x1 - lens.pixel_size / 2, y1 + lens.pixel_size / 2
    return x1.contiguous(), y1.contiguous()


@torch.no_grad()
def sample_sensor(lens, spp=64, pupil=True, wvln=DEFAULT_WAVE, sub_pixel=False):
    """optics.py:497-538: rays [spp, H, W] from the bottom-right corner of every sensor pixel to that pixel's own
    samples of the exit pupil (sample_pupil)."""
    if pupil is not True:
        raise Exception("This feature has been abandoned.")
    if sub_pixel:
        raise Warning("This feature is not finished yet.")
    x1, y1 = sensor_axes(lens)
    x1, y1 = torch.meshgrid(x1, y1, indexing="xy")
    z1 = torch.full_like(x1, lens.d_sensor)
    pupilz, pupilr = lens.exit_pupil()
    o2 = lens.sample_pupil(lens.sensor_res, spp, pupilr=pupilr, pupilz=pupilz)
    o = torch.broadcast_to(torch.stack((x1, y1, z1), 2), o2.shape)
    return Ray(o, o2 - o, wvln=wvln, device=lens.device)


def trace2obj(lens, ray, depth=DEPTH):
    """optics.py:630-635: trace through the lens, then on to the plane z = depth."""
    ray, _, _ = lens.trace(ray)
    return ray.propagate_to(depth)


# ------------------------------------------------------------------------------------ float64 restatement
def _taps_float64(px, py, inv_texel, live, Ht, Wt, fractions=False):
    """The four taps of §7o's lookup in a [Ht, Wt] plane at (px, py) [S, H, W] fp32 with inv_texel texels per mm (rounded
    to fp32 here) -> (idx [4, S, H, W] int64: the taps' offsets in the flattened plane under replicate addressing,
    w [4, S, H, W] float64: w00, w01, w10, w11).  Dead rays land anywhere (NaN included): they are given a texel to
    read with weights of 0 (so that autograd through a read finds no NaN on them), and the caller leaves them out.  The one copy of the
    lookup: the sums and the gradients of this module read through it.  fractions=True: -> (idx, w, fu, fv), the
    lookup's two fractions as float64 (what its derivative in the landing point is made of)."""
    inv = torch.tensor(float(inv_texel), dtype=torch.float32, device=px.device)
    u = Wt / 2 - px * inv                                    # fp32, one rounding per operation
    v = Ht / 2 + py * inv
    a, b = u - 0.5, v - 0.5
    c0, r0 = torch.floor(a), torch.floor(b)
    fu, fv = (a - c0).double(), (b - r0).double()
    c0 = torch.where(live, c0, torch.zeros_like(c0)).clamp(-2, Wt).nan_to_num(nan=0.0).long()
    r0 = torch.where(live, r0, torch.zeros_like(r0)).clamp(-2, Ht).nan_to_num(nan=0.0).long()
    cl, cr = c0.clamp(0, Wt - 1), (c0 + 1).clamp(0, Wt - 1)
    rt, rb = r0.clamp(0, Ht - 1), (r0 + 1).clamp(0, Ht - 1)
    idx = torch.stack((rt * Wt + cl, rt * Wt + cr, rb * Wt + cl, rb * Wt + cr))
    w = torch.stack(((1 - fv) * (1 - fu), (1 - fv) * fu, fv * (1 - fu), fv * fu))
    w = torch.where(live, w, torch.zeros((), dtype=torch.float64, device=px.device))
    return (idx, w, fu, fv) if fractions else (idx, w)


def _read_taps(planes, idx, w, live):
    """planes [N, Ht, Wt] fp32 read through the taps of _taps_float64 -> [N, S, H, W] float64 (0 on dead rays):
    w00 t00 + w01 t01 + w10 t10 + w11 t11, summed left to right."""
    t64 = planes.double().flatten(1)
    t = w[0] * t64[:, idx[0]] + w[1] * t64[:, idx[1]] + w[2] * t64[:, idx[2]] + w[3] * t64[:, idx[3]]
    return torch.where(live, t, torch.zeros((), dtype=torch.float64, device=idx.device))


def _bilinear_float64(planes, px, py, inv_texel, live):
    """§7o's lookup of planes [N, Ht, Wt] fp32 at (px, py) [S, H, W] fp32 with inv_texel texels per mm (rounded to fp32
    here) -> [N, S, H, W] float64.  Dead rays land anywhere (NaN included) and contribute nothing: they are given a
    texel to read and come out as 0."""
    idx, w = _taps_float64(px, py, inv_texel, live, int(planes.shape[-2]), int(planes.shape[-1]))
    return _read_taps(planes, idx, w, live)


def plane_sums_float64(landing, tex, inv_texel, views=None, return_abs=False):
    """The lookup and the sums of DESIGN.md §7o from the rays' landing record, in plain torch (any device).

    landing [5, S, H, W] fp32: px, py, ra, w_L, w_R of every ray ((w_L, w_R) = (sr, sl) of the splat's closed form: the
    image is indexed by sensor position, psf_lr's grids by its negative); tex [T, Ht, Wt] fp32;
    inv_texel: texels per mm on the plane (rounded to fp32 here, as the kernel's argument is).  views: 2 = (L, R) from
    rows 3 and 4, 1 = row 3 only (a call without dual-pixel parameters); None: 2.
    -> num [V, T, H, W], den [V, H, W] float64; with return_abs also the sums of |w ra t_k| [V, T, H, W] (what a
    bound on the summation error is made of)."""
    landing = torch.as_tensor(landing, dtype=torch.float32)
    tex = torch.as_tensor(tex, dtype=torch.float32, device=landing.device)
    V = 2 if views is None else int(views)
    T, Ht, Wt = tex.shape
    px, py, ra = landing[0], landing[1], landing[2]
    live = ra != 0
    t = _bilinear_float64(tex, px, py, inv_texel, live)                                     # [T, S, H, W]
    zero = torch.zeros((), dtype=torch.float64, device=landing.device)
    w = torch.where(live, landing[3:3 + V].double() * ra.double(), zero)                    # [V, S, H, W]
    terms = w[:, None] * t[None]                                                            # [V, T, S, H, W]
    num, den = terms.sum(2), w.sum(1)
    return (num, den, terms.abs().sum(2)) if return_abs else (num, den)


def images_from_sums(num, den, spp=None, photometric=False):
    """num / den where den > 0 and 0 elsewhere (photometric: num / spp), float64; den is broadcast over the planes."""
    if photometric:
        return num / float(spp)
    d = den.unsqueeze(1) if den.dim() == num.dim() - 1 else den
    return torch.where(d > 0, num / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(num))


# ------------------------------------------------------------------------------------ the kernel's host side
def plane_batch(lens, tex, depth, x2, y2, dp=None, wvln=DEFAULT_WAVE, inv_texel=1.0, pixel_center=True, landing=False):
    """ONE launch of the fused kernel (one batch of the Newton trip rule): every pixel of the lens's sensor sends its
    S rays through the pupil points (x2, y2) [S, H, W] at `wvln` and sums tex [T, Ht, Wt] at z = depth.
    -> dict: num [V, T, H, W], den [V, H, W] float64 (V = 2 with dp, else 1), trips (the table the launch finally ran
    with), and with landing=True landing [5, S, H, W]: px, py, ra, w_L, w_R of every ray."""
    lens._require_gpu()
    H, W = (int(v) for v in lens.sensor_res)
    S = int(x2.shape[0])
    T, Ht, Wt = (int(v) for v in tex.shape)
    K = len(lens.surfaces)
    V = 1 if dp is None else 2
    dev = lens.device
    x1, y1 = sensor_axes(lens, pixel_center)
    if tuple(x2.shape) != (S, H, W) or tuple(y2.shape) != (S, H, W):
        raise ValueError(f"pupil points must be [spp, {H}, {W}], got {tuple(x2.shape)} and {tuple(y2.shape)}")
    if tex.dtype != torch.float32 or tex.device != dev:
        raise ValueError("tex must be float32 on the lens's device")
    x2 = x2.to(dev, torch.float32).contiguous()
    y2 = y2.to(dev, torch.float32).contiguous()
    tex = tex.contiguous()
    num = torch.empty((V, T, H, W), dtype=torch.float64, device=dev)
    den = torch.empty((V, H, W), dtype=torch.float64, device=dev)
    land = torch.empty((5, S, H, W), dtype=torch.float32, device=dev) if landing else None
    dpp = None if dp is None else C.byref(_lib.DpParams(*(float(v) for v in dp)))
    pupilz, _ = lens.exit_pupil()
    wv = float(wvln if wvln < 10 else wvln * 1e-3)
    handle = lens.dev_lens(wv)
    flags = lens._math_flags()

    def enqueue(trips, mask_ptr):
        with lens._timed("render_plane"):
            _lib.check(_lib.lib().sdirt_render_plane(
                handle, trips, flags, dptr(x1), dptr(y1), float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz),
                S, H, W, dpp, float(depth), float(inv_texel), dptr(tex), T, Ht, Wt, dptr(num), dptr(den), dptr(land),
                mask_ptr, stream_ptr(dev)))

    key = ("render_plane", round(wv, 6), lens.precision)
    trips = lens._run_with_trips(key, range(K - 1, -1, -1), enqueue)
    out = {"num": num, "den": den, "trips": np.asarray(trips, np.int32)}
    if landing:
        out["landing"] = land
    return out


def _check_render_arguments(lens, img, spp, wvln, pupil_points):
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError("img must be a [B, C, H, W] tensor")
    if img.dtype != torch.float32:
        raise ValueError("img must be float32")
    if int(spp) < 1:
        raise ValueError("spp must be at least 1")
    chroma = not np.isscalar(wvln)
    if chroma and len(wvln) != img.shape[1]:
        raise ValueError(f"{len(wvln)} wavelengths for an image of {img.shape[1]} channels")
    if img.device != lens.device:
        raise ValueError(f"img is on {img.device}, the lens on {lens.device}")
    if pupil_points is not None:
        H, W = lens.sensor_res
        want = ((len(wvln),) if chroma else ()) + (int(spp), int(H), int(W))
        if len(pupil_points) != 2 or any(tuple(p.shape) != want for p in pupil_points):
            raise ValueError(f"pupil_points must be (x2, y2), each of shape {want}")
    return chroma


def render_plane(lens, img, depth, spp=64, dp=None, wvln=DEFAULT_WAVE, scale=None, pixel_center=True,
                 photometric=False, pupil_points=None, return_sums=False, scene_grad=False, dp_grad=False,
                 depth_grad=False):
    """The image(s) the lens forms of the textured plane z = depth (mm, negative), ray traced.

    img [B, C, Ht, Wt] fp32 on the lens's device: the texture, spread over scale x the sensor's extent (scale: object
    height per sensor height, default calc_scale_ray(depth)).  dp = (h, f, w, r): -> (L, R), the two dual-pixel views,
    named as psf_lr names them; dp=None: -> one image with unit weights.  Each [B, C, H, W] fp32 on the lens's sensor
    (sensor_res, sensor_size, pixel_size as they stand), upright: out[i, j] looks at img[i, j].
    wvln: a number -- all B C planes share one trace -- or a sequence of C wavelengths: channel c is traced at wvln[c]
    with a pupil draw of its own (optics.py:764-767).  spp > 64: rounds of 64 samples (the rest in a last, shorter
    one), each a batch of its own for the Newton trip rule; their float64 sums are added.
    pixel_center=False starts the rays at sample_sensor's pixel corners instead of the centres.
    photometric: num / spp instead of num / den (vignetting and dual-pixel shading stay in the image).
    pupil_points=(x2, y2), each [spp, H, W] ([C, spp, H, W] with C wavelengths): the pupil points instead of a draw.
    return_sums: the float64 sums are appended: num [V, B, C, H, W] and den [V, H, W] ([V, C, H, W] with C wavelengths).
    No gradients by default: the call runs without recording, whatever requires one.  scene_grad=True opts in (named
    as local_dp_psf_render_volume names it): in grad mode, with `img` requiring a gradient, the call goes through
    _RenderRecorded and `img` gets the gradient of DESIGN.md §7q (one opaque layer); otherwise scene_grad=True is the
    plain call.  dp_grad=True opts in to the gradient of DESIGN.md §7r in the dual-pixel parameters: h, f, w of dp may
    then be 0-d tensors, and those that require a gradient get one, in their dtype and on their device (r gets none;
    dp=None raises ValueError); the two options compose.  Without dp_grad tensors in dp are turned into floats.
    depth_grad=True opts in to the gradient of DESIGN.md §7s in the plane's position: `depth` and `scale` may then be
    0-d tensors, and those that require a gradient get one, in their dtype and on their device (the derivative of the
    piecewise-bilinear lookup along every ray); it composes with the other two.  With scale=None the default
    calc_scale_ray value is a constant: the texture keeps its extent while the plane moves.  Without depth_grad
    tensors are turned into floats.  return_sums together with a recorded gradient (depth_grad=True included) raises
    ValueError."""
    _check_render_arguments(lens, img, spp, wvln, pupil_points)
    recorded = bool(scene_grad) and torch.is_grad_enabled() and img.requires_grad
    leaves = _dp_leaves(dp, dp_grad)
    zleaves = _depth_leaves(depth, scale, depth_grad)
    if any(v is not None and v.dim() != 0 for v in zleaves):
        raise ValueError("depth_grad=True: depth and scale that take a gradient must be 0-d tensors")
    if torch.is_tensor(depth) and depth.dim() == 0:             # the numbers the forward takes
        depth = _as_floats(depth)
    if torch.is_tensor(scale) and scale.dim() == 0:
        scale = _as_floats(scale)
    tracked = recorded or any(v is not None for v in leaves + zleaves)
    if (tracked or depth_grad) and return_sums:
        raise ValueError("return_sums with a recorded gradient: the float64 sums carry none")
    lens._require_gpu()
    args = (depth, spp, dp, wvln, scale, pixel_center, photometric, pupil_points)
    if tracked:
        res = _recorded_call(lens, img, None, _plane_forward, args, recorded, leaves, zleaves)
        return res if dp is not None else res[0]
    with torch.no_grad():
        return _plane_forward(lens, img, None, *args, return_sums=return_sums)


def _plane_forward(lens, img, alpha, depth, spp, dp, wvln, scale, pixel_center, photometric, pupil_points,
                   return_sums=False, record=None):
    """render_plane behind its argument checks.  record: a dict that receives what _RenderRecorded's backward needs."""
    chroma = not np.isscalar(wvln)
    spp = int(spp)
    B, Cn, Ht, Wt = (int(v) for v in img.shape)
    H, W = (int(v) for v in lens.sensor_res)
    V = 1 if dp is None else 2
    if scale is None:
        scale = lens.calc_scale_ray(depth)
    inv_texel = 1.0 / (float(scale) * lens.pixel_size * W / Wt)
    pupilz, pupilr = lens.exit_pupil()
    # (wavelength, texture planes) of every trace
    if chroma:
        groups = [(wvln[c], img[:, c].contiguous()) for c in range(Cn)]
    else:
        groups = [(wvln, img.reshape(B * Cn, Ht, Wt))]
    nums = [torch.zeros((V, g[1].shape[0], H, W), dtype=torch.float64, device=lens.device) for g in groups]
    dens = [torch.zeros((V, H, W), dtype=torch.float64, device=lens.device) for _ in groups]
    for s0 in range(0, spp, CHUNK_SPP):
        n = min(CHUNK_SPP, spp - s0)
        for g, (wv, tex) in enumerate(groups):
            if pupil_points is None:
                o2 = lens.sample_pupil((H, W), n, pupilr=pupilr, pupilz=pupilz)
                x2, y2 = o2[..., 0], o2[..., 1]
            else:
                x2, y2 = (p[g, s0:s0 + n] if chroma else p[s0:s0 + n] for p in pupil_points)
            part = plane_batch(lens, tex, depth, x2, y2, dp, wv, inv_texel, pixel_center)
            nums[g] += part["num"]
            dens[g] += part["den"]
            if record is not None:
                record["chunks"].append((g, x2.to(lens.device, torch.float32), y2.to(lens.device, torch.float32),
                                         part["trips"]))
    if record is not None:
        record.update(wv=[g[0] for g in groups], den=dens, num=nums, depths=[float(depth)], inv_texels=[inv_texel],
                      scales=[float(scale)], dp=dp, pixel_center=pixel_center, spp=spp, photometric=photometric,
                      chroma=chroma, plane=True)
    if chroma:
        num, den = torch.stack(nums, 2), torch.stack(dens, 1)               # [V, B, C, H, W], [V, C, H, W]
        den_b = den.unsqueeze(1)
    else:
        num, den = nums[0].view(V, B, Cn, H, W), dens[0]
        den_b = den.view(V, 1, 1, H, W)
    out = images_from_sums(num, den_b, spp, photometric).float()
    res = (out[0], out[1]) if dp is not None else (out[0],)
    if return_sums:
        res = res + (num, den)
    return res if len(res) > 1 else res[0]


# ------------------------------------------------------------------------------------ a stack of layers
def layer_sums_float64(landing, alpha, tex, inv_texels, views=None, return_abs=False):
    """The lookups, the compositing and the sums of DESIGN.md §7p from the rays' landing record, in plain torch.

    landing [3 + 2 L, S, H, W] fp32: ra, w_L, w_R, then (px_l, py_l) of every layer; alpha [L, Ht, Wt] fp32; tex
    [L, T, Ht, Wt] fp32, or [T, Ht, Wt] shared by all layers; inv_texels: L numbers, texels per mm on every layer
    (rounded to fp32 here).  views as in plane_sums_float64 (rows 1 and 2).
    -> num [V, T, H, W], den [V, H, W], cov [V, H, W] float64; with return_abs also the sums of |wr c_k| [V, T, H, W]
    and of |wr o| [V, H, W]."""
    landing = torch.as_tensor(landing, dtype=torch.float32)
    dev = landing.device
    alpha = torch.as_tensor(alpha, dtype=torch.float32, device=dev)
    tex = torch.as_tensor(tex, dtype=torch.float32, device=dev)
    V = 2 if views is None else int(views)
    L = int(alpha.shape[0])
    if landing.shape[0] != 3 + 2 * L or len(inv_texels) != L:
        raise ValueError(f"{L} layers need a landing record of {3 + 2 * L} rows and {L} inv_texels")
    if tex.dim() == 3:
        tex = tex.unsqueeze(0).expand(L, *tex.shape)
    ra = landing[0]
    live = ra != 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    T = torch.ones(ra.shape, dtype=torch.float64, device=dev)
    c = torch.zeros((tex.shape[1],) + tuple(ra.shape), dtype=torch.float64, device=dev)
    for l in range(L):
        px, py = landing[3 + 2 * l], landing[4 + 2 * l]
        a = _bilinear_float64(alpha[l:l + 1], px, py, inv_texels[l], live)[0]
        t = _bilinear_float64(tex[l], px, py, inv_texels[l], live)
        g = T * a
        c = c + g * t
        T = T * (1 - a)
    o = 1 - T
    w = torch.where(live, landing[1:1 + V].double() * ra.double(), zero)                    # [V, S, H, W]
    terms = torch.where(live, w[:, None] * c[None], zero)                                   # [V, T, S, H, W]
    oterms = torch.where(live, w * o, zero)
    num, den, cov = terms.sum(2), w.sum(1), oterms.sum(1)
    return (num, den, cov, terms.abs().sum(2), oterms.abs().sum(1)) if return_abs else (num, den, cov)


def _check_layers(alpha, tex, depths, inv_texels=None, scan=True):
    """The scene of §7p: -> (L, T, Ht, Wt, shared).  alpha [L, Ht, Wt] in [0, 1], tex [L, T, Ht, Wt] or [T, Ht, Wt].
    scan=False leaves out the one check that reads alpha (and so waits for the device): its range."""
    if not torch.is_tensor(alpha) or alpha.dim() != 3:
        raise ValueError("alpha must be a [L, Ht, Wt] tensor")
    if not torch.is_tensor(tex) or tex.dim() not in (3, 4):
        raise ValueError("the layers' image must be a [L, C, Ht, Wt] tensor, or [C, Ht, Wt] shared by all layers")
    if alpha.dtype != torch.float32 or tex.dtype != torch.float32:
        raise ValueError("alpha and the layers' image must be float32")
    L, Ht, Wt = (int(v) for v in alpha.shape)
    if not 1 <= L <= _lib.MAX_LAYERS:
        raise ValueError(f"{L} layers: between 1 and {_lib.MAX_LAYERS} are supported")
    shared = tex.dim() == 3
    if tuple(tex.shape[-2:]) != (Ht, Wt) or (not shared and int(tex.shape[0]) != L):
        raise ValueError(f"alpha is {tuple(alpha.shape)}, the layers' image {tuple(tex.shape)}: layers or extents differ")
    depths = [float(d) for d in depths]
    if len(depths) != L or (inv_texels is not None and len(inv_texels) != L):
        raise ValueError(f"{L} layers need {L} depths and {L} scales")
    z = np.asarray(depths, np.float32)
    if not (z[0] < 0 and bool((z[1:] < z[:-1]).all())):
        raise ValueError("layer depths must be negative and strictly descending (the nearest layer first)")
    if scan and alpha.device.type != "meta" and alpha.numel() and not bool(((alpha >= 0) & (alpha <= 1)).all()):
        raise ValueError("alpha must lie in [0, 1]")
    return L, int(tex.shape[-3]), Ht, Wt, shared


def layer_batch(lens, alpha, tex, depths, inv_texels, x2, y2, dp=None, wvln=DEFAULT_WAVE, pixel_center=True,
                landing=False, check_alpha=True):
    """ONE launch of the layered kernel (one batch of the Newton trip rule): plane_batch with a stack of layers.
    alpha [L, Ht, Wt], tex [L, T, Ht, Wt] (or [T, Ht, Wt] shared by all layers: layer stride 0), depths and inv_texels
    L numbers each, the nearest layer first.
    -> dict: num [V, T, H, W], den, cov [V, H, W] float64, trips, and landing ([3 + 2 L, S, H, W]: ra, w_L, w_R, px_0,
    py_0, ...) or None.  check_alpha=False: the caller has verified that alpha lies in [0, 1] (render_layers does, once
    per call and not once per launch: the check reads all of alpha and waits for the device)."""
    L, T, Ht, Wt, shared = _check_layers(alpha, tex, depths, inv_texels, scan=check_alpha)
    lens._require_gpu()
    H, W = (int(v) for v in lens.sensor_res)
    S = int(x2.shape[0])
    K = len(lens.surfaces)
    V = 1 if dp is None else 2
    dev = lens.device
    x1, y1 = sensor_axes(lens, pixel_center)
    if tuple(x2.shape) != (S, H, W) or tuple(y2.shape) != (S, H, W):
        raise ValueError(f"pupil points must be [spp, {H}, {W}], got {tuple(x2.shape)} and {tuple(y2.shape)}")
    if tex.device != dev or alpha.device != dev:
        raise ValueError("alpha and tex must be on the lens's device")
    x2 = x2.to(dev, torch.float32).contiguous()
    y2 = y2.to(dev, torch.float32).contiguous()
    alpha, tex = alpha.contiguous(), tex.contiguous()
    num = torch.empty((V, T, H, W), dtype=torch.float64, device=dev)
    den = torch.empty((V, H, W), dtype=torch.float64, device=dev)
    cov = torch.empty((V, H, W), dtype=torch.float64, device=dev)
    land = torch.empty((3 + 2 * L, S, H, W), dtype=torch.float32, device=dev) if landing else None
    dpp = None if dp is None else C.byref(_lib.DpParams(*(float(v) for v in dp)))
    z = (C.c_double * L)(*(float(d) for d in depths))
    inv = (C.c_double * L)(*(float(v) for v in inv_texels))
    pupilz, _ = lens.exit_pupil()
    wv = float(wvln if wvln < 10 else wvln * 1e-3)
    handle = lens.dev_lens(wv)
    flags = lens._math_flags()

    def enqueue(trips, mask_ptr):
        with lens._timed("render_layers"):
            _lib.check(_lib.lib().sdirt_render_layers(
                handle, trips, flags, dptr(x1), dptr(y1), float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz),
                S, H, W, dpp, L, z, inv, dptr(alpha), dptr(tex), 0 if shared else T * Ht * Wt, T, Ht, Wt, dptr(num),
                dptr(den), dptr(cov), dptr(land), mask_ptr, stream_ptr(dev)))

    key = ("render_layers", round(wv, 6), lens.precision)
    trips = lens._run_with_trips(key, range(K - 1, -1, -1), enqueue)
    return {"num": num, "den": den, "cov": cov, "trips": np.asarray(trips, np.int32), "landing": land}


def render_layers(lens, img, alpha, depths, spp=64, dp=None, wvln=DEFAULT_WAVE, scales=None, pixel_center=True,
                  photometric=False, pupil_points=None, return_sums=False, scene_grad=False, dp_grad=False,
                  depth_grad=False):
    """The image(s) the lens forms of a stack of fronto-parallel layers, ray traced with occlusion.

    img [L, C, Ht, Wt] fp32, or [C, Ht, Wt] shared by all layers; alpha [L, Ht, Wt] fp32 in [0, 1]: layer l covers the
    ray by alpha[l] where the ray meets z = depths[l]; depths (mm): 0 > depths[0] > depths[1] > ..., the nearest first.
    Every layer is spread over scales[l] x the sensor's extent (default calc_scale_ray(depths[l]): the layers register
    on the sensor under perspective).  Along a ray the layers are composited front to back; what passes every layer is
    black.  dp, wvln (a number or C wavelengths), spp > 64, pixel_center, photometric and pupil_points as in
    render_plane.  -> (L, R) with dp, else one image, each [C, H, W] fp32.
    return_sums: num [V, C, H, W], den and cov [V, H, W] ([V, C, H, W] with C wavelengths) are appended; cov / den is
    the share of a pixel's light that met some layer.
    No gradients by default.  scene_grad=True opts in: in grad mode, with `img` or `alpha` requiring a gradient, the
    call goes through _RenderRecorded and both get the gradient of DESIGN.md §7q (fp32, of their own shape; a shared
    image gets the sum over its layers); otherwise scene_grad=True is the plain call.  dp, the lens, depths, scales and
    pupil_points get none.  dp_grad=True opts in to the gradient of DESIGN.md §7r: h, f, w of dp may then be 0-d
    tensors, and those that require a gradient get one, in their dtype and on their device (r gets none; dp=None raises
    ValueError); the two options compose, one backward running both kernels from the one record.
    depth_grad=True opts in to the gradient of DESIGN.md §7s in the layers' positions: `depths` and `scales` may then
    each be a 1-D tensor of L, and those that require a gradient get one, in their dtype and on their device.  It is
    the derivative of the piecewise-bilinear lookups along every ray, pushed through the compositing: on a hard matte
    it lives on the transition texels of alpha.  With scales=None the default calc_scale_ray values are constants:
    every layer keeps its extent while it moves.  A caller who wants the layers to stay registered on the sensor
    builds `scales` from the depth tensor (a pinhole: scale proportional to -depth), and autograd chains the two.
    It composes with scene_grad and dp_grad: one backward runs the kernels from the one record.  Without depth_grad
    tensors are turned into floats.  return_sums together with a recorded gradient (depth_grad=True included) raises
    ValueError."""
    if not torch.is_tensor(img) or img.dim() not in (3, 4):
        raise ValueError("img must be a [L, C, Ht, Wt] tensor, or [C, Ht, Wt] shared by all layers")
    if scales is not None and len(scales) != len(depths):
        raise ValueError(f"{len(scales)} scales for {len(depths)} depths")
    zleaves = _depth_leaves(depths, scales, depth_grad)
    if any(v is not None and v.dim() != 1 for v in zleaves):
        raise ValueError(f"depth_grad=True: depths and scales that take a gradient must be 1-D tensors of {len(depths)}")
    if torch.is_tensor(depths) and depths.dim() == 1:           # the numbers the forward takes (no gradient is lost:
        depths = _as_floats(depths)                             # zleaves holds the tensors that take one)
    if torch.is_tensor(scales) and scales.dim() == 1:
        scales = _as_floats(scales)
    L, Cn, Ht, Wt, shared = _check_layers(alpha, img, depths)
    chroma = _check_render_arguments(lens, img.unsqueeze(0) if shared else img, spp, wvln, pupil_points)
    if alpha.device != lens.device:
        raise ValueError(f"alpha is on {alpha.device}, the lens on {lens.device}")
    recorded = bool(scene_grad) and torch.is_grad_enabled() and (img.requires_grad or alpha.requires_grad)
    leaves = _dp_leaves(dp, dp_grad)
    tracked = recorded or any(v is not None for v in leaves + zleaves)
    if (tracked or depth_grad) and return_sums:
        raise ValueError("return_sums with a recorded gradient: the float64 sums carry none")
    lens._require_gpu()
    args = (depths, spp, dp, wvln, scales, pixel_center, photometric, pupil_points)
    if tracked:
        res = _recorded_call(lens, img, alpha, _layers_forward, args, recorded, leaves, zleaves)
        return res if dp is not None else res[0]
    with torch.no_grad():
        return _layers_forward(lens, img, alpha, *args, return_sums=return_sums)


def _layers_forward(lens, img, alpha, depths, spp, dp, wvln, scales, pixel_center, photometric, pupil_points,
                    return_sums=False, record=None):
    """render_layers behind its argument checks.  record: a dict that receives what _RenderRecorded's backward needs."""
    L, Cn, Ht, Wt, shared = _check_layers(alpha, img, depths, scan=False)
    chroma = not np.isscalar(wvln)
    spp = int(spp)
    H, W = (int(v) for v in lens.sensor_res)
    V = 1 if dp is None else 2
    if scales is None:
        scales = scale_per_layer(lens, depths)
    inv_texels = [1.0 / (float(s) * lens.pixel_size * W / Wt) for s in scales]
    pupilz, pupilr = lens.exit_pupil()
    if chroma:
        groups = [(wvln[c], img[c:c + 1] if shared else img[:, c:c + 1].contiguous()) for c in range(Cn)]
    else:
        groups = [(wvln, img)]
    nums = [torch.zeros((V, g[1].shape[-3], H, W), dtype=torch.float64, device=lens.device) for g in groups]
    dens = [torch.zeros((V, H, W), dtype=torch.float64, device=lens.device) for _ in groups]
    covs = [torch.zeros((V, H, W), dtype=torch.float64, device=lens.device) for _ in groups]
    for s0 in range(0, spp, CHUNK_SPP):
        n = min(CHUNK_SPP, spp - s0)
        for g, (wv, tex) in enumerate(groups):
            if pupil_points is None:
                o2 = lens.sample_pupil((H, W), n, pupilr=pupilr, pupilz=pupilz)
                x2, y2 = o2[..., 0], o2[..., 1]
            else:
                x2, y2 = (p[g, s0:s0 + n] if chroma else p[s0:s0 + n] for p in pupil_points)
            part = layer_batch(lens, alpha, tex, depths, inv_texels, x2, y2, dp, wv, pixel_center, check_alpha=False)
            nums[g] += part["num"]
            dens[g] += part["den"]
            covs[g] += part["cov"]
            if record is not None:
                record["chunks"].append((g, x2.to(lens.device, torch.float32), y2.to(lens.device, torch.float32),
                                         part["trips"]))
    if record is not None:
        record.update(wv=[g[0] for g in groups], den=dens, num=nums, depths=[float(d) for d in depths], inv_texels=inv_texels,
                      scales=[float(s) for s in scales], dp=dp, pixel_center=pixel_center, spp=spp,
                      photometric=photometric, chroma=chroma, plane=False)
    if chroma:
        num, den, cov = torch.cat(nums, 1), torch.stack(dens, 1), torch.stack(covs, 1)     # [V, C, H, W] each
        den_b = den
    else:
        num, den, cov = nums[0], dens[0], covs[0]
        den_b = den.unsqueeze(1)
    out = images_from_sums(num, den_b, spp, photometric).float()
    res = (out[0], out[1]) if dp is not None else (out[0],)
    if return_sums:
        res = res + (num, den, cov)
    return res if len(res) > 1 else res[0]


def scale_per_layer(lens, depths):
    """calc_scale_ray of every layer depth (each traces randomly drawn rays of its own)."""
    return [lens.calc_scale_ray(float(d)) for d in depths]


def layers_from_rgbd(depth, layer_depths, extend=True):
    """Cut a depth map into the coverage maps of a layer stack: depth [H, W] (or [1, H, W]; mm, negative),
    layer_depths: L depths, the nearest first -> alpha [L, H, W] fp32 of zeros and ones on depth's device.
    Every pixel belongs to the layer nearest to it in 1 / depth (of two equally near ones, to the nearer to the lens).
    extend: the pixel also covers every layer BEHIND its own, so the last layer is opaque, no ray falls through a
    disocclusion (it meets what the occluder's own surroundings show there) and cov == den; without it alpha is
    one-hot over the layers."""
    depth = torch.as_tensor(depth)
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2:
        raise ValueError("depth must be [H, W] or [1, H, W]")
    z = torch.as_tensor([float(d) for d in layer_depths], dtype=torch.float64, device=depth.device)
    if z.numel() < 1 or not (bool((z < 0).all()) and bool((z[1:] < z[:-1]).all())):
        raise ValueError("layer depths must be negative and strictly descending (the nearest layer first)")
    if depth.device.type != "meta" and not bool((depth < 0).all()):
        raise ValueError("depth must be negative (mm in front of the lens)")
    dist = (1.0 / depth.double()[None] - 1.0 / z[:, None, None]).abs()                     # [L, H, W]
    own = dist.argmin(0)                                       # the first of equal minima: the nearer layer
    idx = torch.arange(z.numel(), device=depth.device)[:, None, None]
    return ((idx >= own[None]) if extend else (idx == own[None])).float()


def uniform_layer_depths(depth, n_layers):
    """Up to n_layers depths uniform in 1 / depth from the nearest to the farthest value of `depth` (mm, negative), the
    nearest first.  The kernel carries its rays to depths rounded to fp32, so layers whose depths are equal after that
    rounding are one layer: a map of one depth, or of a range below fp32's resolution, gives fewer layers than asked for."""
    near, far = float(depth.max()), float(depth.min())
    if int(n_layers) == 1 and near != far:
        return [2.0 / (1.0 / near + 1.0 / far)]
    inv = np.linspace(1.0 / near, 1.0 / far, int(n_layers))
    zs = [near] + [float(1.0 / v) for v in inv[1:-1]] + [far]
    out = []
    for z in zs:
        if not out or np.float32(z) < np.float32(out[-1]):
            out.append(z)
    return out


def render_rgbd(lens, img, depth, layer_depths=None, n_layers=8, spp=64, dp=None, wvln=DEFAULT_WAVE, scales=None,
                pixel_center=True, photometric=False, pupil_points=None, extend=True, scene_grad=False, dp_grad=False,
                depth_grad=False):
    """The ray-traced dual-pixel pair of an RGB-D frame -- the input PSFNet.render takes -- with occlusion: img
    [B, C, H, W] fp32, depth [B, 1, H, W] (mm, negative).  Every frame is cut into layers by layers_from_rgbd (at
    layer_depths, or at n_layers depths uniform in 1 / depth between the frame's nearest and farthest) that all show
    the frame's image, and rendered by render_layers: one call per batch element, the other arguments as there (default
    scales: calc_scale_ray once per distinct stack of depths, so frames that share their layers register alike).
    -> (L, R) with dp, else one image, each [B, C, H, W] fp32.
    No gradients by default.  scene_grad=True: render_layers' -- img[b], which all layers of frame b show, gets the
    gradient summed over its layers; `depth` gets none (layers_from_rgbd is a hard assignment).  dp_grad=True:
    render_layers' -- h, f, w get the sum over the batch.  depth_grad=True: render_layers' -- `layer_depths` and
    `scales`, given as 1-D tensors, get the sum over the batch; the depth MAP still gets none, and so
    do depths that uniform_layer_depths made of it."""
    if dp_grad and dp is None:
        raise ValueError("dp_grad=True with dp=None: one view with unit weights has no sub-pixel model")
    with torch.set_grad_enabled((bool(scene_grad) or bool(dp_grad) or bool(depth_grad)) and torch.is_grad_enabled()):
        return _render_rgbd(lens, img, depth, layer_depths, n_layers, spp, dp, wvln, scales, pixel_center, photometric,
                            pupil_points, extend, scene_grad, dp_grad, depth_grad)


def _render_rgbd(lens, img, depth, layer_depths, n_layers, spp, dp, wvln, scales, pixel_center, photometric,
                 pupil_points, extend, scene_grad, dp_grad=False, depth_grad=False):
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError("img must be a [B, C, H, W] tensor")
    if not torch.is_tensor(depth) or depth.dim() != 4 or depth.shape[1] != 1 or depth.shape[0] != img.shape[0] \
            or depth.shape[-2:] != img.shape[-2:]:
        raise ValueError(f"depth must be [B, 1, H, W] for an image of {tuple(img.shape)}")
    if int(n_layers) < 1 or int(n_layers) > _lib.MAX_LAYERS:
        raise ValueError(f"n_layers must be between 1 and {_lib.MAX_LAYERS}")
    views, scales_of = [], {}
    for b in range(img.shape[0]):
        zs = uniform_layer_depths(depth[b, 0], n_layers) if layer_depths is None else _as_floats(layer_depths)
        alpha = layers_from_rgbd(depth[b, 0].detach(), zs, extend).to(img.device)
        if scales is None and tuple(zs) not in scales_of:      # calc_scale_ray traces rays of its own: once per stack
            scales_of[tuple(zs)] = scale_per_layer(lens, zs)
        moving = depth_grad and torch.is_tensor(layer_depths)     # the tensor itself goes on: it may take a gradient
        out = render_layers(lens, img[b], alpha, layer_depths if moving else zs, spp=spp, dp=dp, wvln=wvln,
                            scales=scales_of[tuple(zs)] if scales is None else scales,
                            pixel_center=pixel_center, photometric=photometric, pupil_points=pupil_points,
                            scene_grad=scene_grad, dp_grad=dp_grad, depth_grad=depth_grad)
        views.append(out if dp is not None else (out,))
    res = tuple(torch.stack(v) for v in zip(*views))
    return res if dp is not None else res[0]


# ------------------------------------------------------------------------------------ gradients
def layer_grads_float64(landing, alpha, tex, inv_texels, gnum, views=None, return_abs=False):
    """The adjoint of DESIGN.md §7q from the rays' landing record, in plain torch and without autograd: what
    sdirt_render_layers_grad adds to zeroed buffers, every term in the kernel's bits, the terms of a texel summed in
    index_add_'s order.

    landing, alpha, tex, inv_texels, views as in layer_sums_float64; alpha=None: every layer opaque (no coverage
    gradient); gnum [V, T, H, W] float64: the adjoint of num.
    -> galpha [L, Ht, Wt] (None without alpha), gtex of tex's shape (a shared [T, Ht, Wt] gets the sum over the layers),
    float64; with return_abs also the sums of |term| of both, absolute values taken before any cancellation: colour
    |q|_k g_l w_j with |q|_k = sum_side wr |gnum|, coverage T_l (Dbar_l + Rbar_{l+1}) w_j with Dbar_l = sum_k |q|_k
    |t_{l,k}| and Rbar the recursion of R on Dbar."""
    landing = torch.as_tensor(landing, dtype=torch.float32)
    dev = landing.device
    tex = torch.as_tensor(tex, dtype=torch.float32, device=dev)
    gnum = torch.as_tensor(gnum, dtype=torch.float64, device=dev)
    V = 2 if views is None else int(views)
    L = len(inv_texels)
    if landing.shape[0] != 3 + 2 * L:
        raise ValueError(f"{L} layers need a landing record of {3 + 2 * L} rows and {L} inv_texels")
    opaque = alpha is None
    if not opaque:
        alpha = torch.as_tensor(alpha, dtype=torch.float32, device=dev)
        if alpha.shape[0] != L:
            raise ValueError(f"alpha has {alpha.shape[0]} layers, inv_texels {L}")
    shared = tex.dim() == 3
    NT, Ht, Wt = (int(v) for v in tex.shape[-3:])
    if tuple(gnum.shape) != (V, NT) + tuple(landing.shape[2:]):
        raise ValueError(f"gnum must be {(V, NT) + tuple(landing.shape[2:])}, got {tuple(gnum.shape)}")
    ra = landing[0]
    live = ra != 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    wr = torch.where(live, landing[1:1 + V].double() * ra.double(), zero)                   # [V, S, H, W]
    q = wr[0] * gnum[0][:, None]                                                            # [T, S, H, W]
    qa = wr[0] * gnum[0].abs()[:, None]
    if V == 2:
        q, qa = q + wr[1] * gnum[1][:, None], qa + wr[1] * gnum[1].abs()[:, None]
    gtex = torch.zeros(tex.shape, dtype=torch.float64, device=dev)
    gtex_abs = torch.zeros_like(gtex)
    galpha = None if opaque else torch.zeros(alpha.shape, dtype=torch.float64, device=dev)
    galpha_abs = None if opaque else torch.zeros_like(galpha)

    def scatter(buf, idx, w, val, sel):
        flat = buf.view(-1)
        for j in range(4):
            flat.index_add_(0, idx[j][sel], (val * w[j])[sel])

    T = torch.ones(ra.shape, dtype=torch.float64, device=dev)
    kept = []
    for l in range(L):
        idx, w = _taps_float64(landing[3 + 2 * l], landing[4 + 2 * l], inv_texels[l], live, Ht, Wt)
        a = torch.ones_like(T) if opaque else _read_taps(alpha[l:l + 1], idx, w, live)[0]
        t = _read_taps(tex if shared else tex[l], idx, w, live)
        g = T * a
        D, Dbar = q[0] * t[0], qa[0] * t[0].abs()
        for k in range(1, NT):
            D, Dbar = D + q[k] * t[k], Dbar + qa[k] * t[k].abs()
        sel = live & (g != 0)
        for k in range(NT):
            scatter(gtex[k] if shared else gtex[l, k], idx, w, q[k] * g, sel)
            scatter(gtex_abs[k] if shared else gtex_abs[l, k], idx, w, qa[k] * g, sel)
        kept.append((idx, w, a, D, Dbar, T))
        T = T * (1 - a)
    if not opaque:
        R, Rbar = torch.zeros_like(T), torch.zeros_like(T)
        for l in range(L - 1, -1, -1):
            idx, w, a, D, Dbar, Tl = kept[l]
            d = D - R
            sel = live & (Tl != 0)
            scatter(galpha[l], idx, w, Tl * d, sel)
            scatter(galpha_abs[l], idx, w, Tl * (Dbar + Rbar), sel)
            R, Rbar = R + a * d, a * Dbar + (1 - a) * Rbar
    return (galpha, gtex, galpha_abs, gtex_abs) if return_abs else (galpha, gtex)


def gnum_from_image_grad(G, den_total, spp=None, photometric=False):
    """The adjoint of the float64 sums `num` from the adjoint G of the image(s) images_from_sums made of them:
    G / den_total where den_total > 0 and 0 elsewhere (photometric: G / spp), float64.  G [V, ..., H, W] of any float
    dtype, den_total [V, H, W]: the TOTAL over every chunk of samples, broadcast over the dimensions between."""
    G = G.double()
    if photometric:
        return G / float(spp)
    d = den_total.view(den_total.shape[:1] + (1,) * (G.dim() - den_total.dim()) + den_total.shape[1:])
    return torch.where(d > 0, G / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(G))


def layer_grad_batch(lens, alpha, tex, depths, inv_texels, x2, y2, trips, gnum, dp=None, wvln=DEFAULT_WAVE,
                     pixel_center=True, galpha=None, gtex=None):
    """ONE call of sdirt_render_layers_grad: the counterpart of layer_batch (same scene, pupil points, dp, wvln and
    pixel_center), with `trips` the table that call ended with (its "trips") and gnum [V, T, H, W] float64 the adjoint
    of its num.  alpha=None: every layer opaque (render_plane's scene with L = 1), no coverage gradient.
    galpha [L, Ht, Wt], gtex (tex's shape) float64 on the lens's device: the buffers the gradients are ADDED to; None:
    a zeroed one is made; False: that gradient is not wanted.  -> (galpha, gtex), None where not wanted.
    The adds are float64 atomics: two calls need not agree in every bit."""
    dev = lens.device
    if alpha is None:
        if not torch.is_tensor(tex) or tex.dim() not in (3, 4) or tex.dtype != torch.float32:
            raise ValueError("the layers' image must be a float32 [L, C, Ht, Wt] tensor, or [C, Ht, Wt] shared by all layers")
        shared = tex.dim() == 3
        L, (T, Ht, Wt) = len(depths), (int(v) for v in tex.shape[-3:])
        if not 1 <= L <= _lib.MAX_LAYERS or len(inv_texels) != L or (not shared and int(tex.shape[0]) != L):
            raise ValueError(f"{L} depths, {len(inv_texels)} scales and an image of {tuple(tex.shape)}: layers differ")
        if galpha is not None and galpha is not False:
            raise ValueError("an opaque stack (alpha=None) has no coverage gradient")
        galpha = False
    else:
        L, T, Ht, Wt, shared = _check_layers(alpha, tex, depths, inv_texels, scan=False)
        if alpha.device != dev:
            raise ValueError("alpha and tex must be on the lens's device")
        alpha = alpha.contiguous()
    if tex.device != dev:
        raise ValueError("alpha and tex must be on the lens's device")
    if galpha is False and gtex is False:
        raise ValueError("galpha and gtex are both False: no gradient is asked for")
    H, W = (int(v) for v in lens.sensor_res)
    S = int(x2.shape[0])
    K = len(lens.surfaces)
    V = 1 if dp is None else 2
    if tuple(x2.shape) != (S, H, W) or tuple(y2.shape) != (S, H, W):
        raise ValueError(f"pupil points must be [spp, {H}, {W}], got {tuple(x2.shape)} and {tuple(y2.shape)}")
    if len(trips) != K:
        raise ValueError(f"{len(trips)} trip counts for a lens of {K} surfaces")
    if not torch.is_tensor(gnum) or gnum.dtype != torch.float64 or gnum.device != dev or tuple(gnum.shape) != (V, T, H, W):
        raise ValueError(f"gnum must be float64 {(V, T, H, W)} on the lens's device")

    def buffer(given, like, name):
        if given is False:
            return None
        if given is None:
            return torch.zeros(like.shape, dtype=torch.float64, device=dev)
        if not torch.is_tensor(given) or given.dtype != torch.float64 or given.device != dev \
                or given.shape != like.shape or not given.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float64 {tuple(like.shape)} on the lens's device")
        return given

    lens._require_gpu()
    galpha = buffer(galpha, alpha, "galpha")
    gtex = buffer(gtex, tex, "gtex")
    x1, y1 = sensor_axes(lens, pixel_center)
    x2 = x2.to(dev, torch.float32).contiguous()
    y2 = y2.to(dev, torch.float32).contiguous()
    tex, gnum = tex.contiguous(), gnum.contiguous()
    dpp = None if dp is None else C.byref(_lib.DpParams(*(float(v) for v in dp)))
    z = (C.c_double * L)(*(float(d) for d in depths))
    inv = (C.c_double * L)(*(float(v) for v in inv_texels))
    pupilz, _ = lens.exit_pupil()
    wv = float(wvln if wvln < 10 else wvln * 1e-3)
    stride = 0 if shared else T * Ht * Wt
    with lens._timed("render_layers_grad"):
        _lib.check(_lib.lib().sdirt_render_layers_grad(
            lens.dev_lens(wv), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
            float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), S, H, W, dpp, L, z, inv, dptr(alpha), dptr(tex),
            stride, T, Ht, Wt, dptr(gnum), dptr(galpha), dptr(gtex), stride, stream_ptr(dev)))
    return galpha, gtex


# ------------------------------------------------------------------------------------ gradients in h, f, w
def gden_from_image_grad(G, num_total, den_total, photometric=False):
    """The adjoint of the float64 sums `den` from the adjoint G of the image(s) num / den:
    gden[side] = -sum_k G[side, k] num_total[side, k] / den_total[side]^2 where den_total > 0 and 0 elsewhere, float64
    [V, H, W]; the sum runs over every dimension between the view and the pixel.  G and num_total [V, ..., H, W],
    den_total [V, H, W]: the TOTALS over every chunk of samples.  photometric: the image is num / spp, den has no
    adjoint: -> None."""
    if photometric:
        return None
    G, num_total = G.double(), num_total.double()
    if G.shape != num_total.shape or G.dim() < 3 or tuple(den_total.shape) != (G.shape[0],) + tuple(G.shape[-2:]):
        raise ValueError(f"G and num_total must be one [V, ..., H, W], den_total [V, H, W]; got {tuple(G.shape)}, "
                         f"{tuple(num_total.shape)} and {tuple(den_total.shape)}")
    s = (G * num_total).reshape(G.shape[0], -1, *G.shape[-2:]).sum(1)
    ok = den_total > 0
    d = torch.where(ok, den_total, torch.ones_like(den_total))
    return torch.where(ok, -s / (d * d), torch.zeros_like(s))


def _dz_float64(t, h, f, w, r):
    """d/d(h, f, w) of the three boundaries' Z_a (a = +1, 0, -1: right, middle, left) of the sub-pixel model at
    x_tan = t (float64, any shape) -> [3 (a), 3 (h, f, w), ...] float64, by the formulas of DESIGN.md §7r: with x1 the
    boundary projected through the microlens, x2 the margin boundary and A'(x) = -2 sqrt(max((r - x)(r + x), 0)),
      r <= 0.5:  dZ = [|x1| <= r] A'(x1) dx1 + [|x2| <= 0.5] (-1 - [|x2| <= r] A'(x2)) dx2
      r >  0.5:  dZ = [|x1| <= 0.5] T'(x1) dx1 + [|x2| <= 0.5] (-1 - T'(x2)) dx2,  T'(x) = -1 where |x| <= sqrt(r^2 - 1/4),
                 else A'(x)
      dx1 = (-u f / D^2, -h t / D + u h / D^2, a f / D),  u = f t - a w,  D = f - h;      dx2 = (-t, 0, a).
    Every decision is taken in float64 here, by the kernel on the forward's fp32 values: a ray within rounding of
    |x2| = 0.5 (or, r > 0.5, |x1| = 0.5), where the derivative jumps, can come out on the other side."""
    D = f - h
    zero = torch.zeros_like(t)

    def chord(x):
        return -2.0 * torch.sqrt(torch.clamp((r - x) * (r + x), min=0.0))

    rows = []
    for a in (1.0, 0.0, -1.0):
        u = f * t - a * w
        x1 = a * w - u * h / D
        x2 = a * w - h * t
        if r <= 0.5:
            c1 = torch.where(x1.abs() <= r, chord(x1), zero)
            c2 = torch.where(x2.abs() <= 0.5, -1.0 - torch.where(x2.abs() <= r, chord(x2), zero), zero)
        else:
            edge = (r * r - 0.25) ** 0.5
            c1 = torch.where(x1.abs() <= 0.5, torch.where(x1.abs() <= edge, -torch.ones_like(t), chord(x1)), zero)
            c2 = torch.where(x2.abs() <= 0.5, -1.0 - torch.where(x2.abs() <= edge, -torch.ones_like(t), chord(x2)), zero)
        d1 = (-u * f / (D * D), -h * t / D + u * h / (D * D), a * f / D + zero)
        d2 = (-t, zero, a + zero)
        rows.append(torch.stack([c1 * d1[j] + c2 * d2[j] for j in range(3)]))
    return torch.stack(rows)


def layer_dp_grads_float64(landing, x_tan, alpha, tex, inv_texels, gnum, gden, dp, return_abs=False):
    """The adjoint of DESIGN.md §7r from the forward's landing record, in plain torch and without autograd: what
    sdirt_render_layers_dp_grad's partial rows add up to.

    landing, alpha (None: every layer opaque), tex, inv_texels as in layer_sums_float64; x_tan [S, H, W] fp32: the
    kernel's x_tan of every ray; gnum [2, T, H, W], gden [2, H, W] or None, float64; dp = (h, f, w, r).
    Per live ray: c_k by the forward's walk (a layer behind T == 0 is not read), A_side = ra (gnum[side, 0] c_0 + ... +
    gden[side]), and the term A_0 dw_L + A_1 dw_R with (w_L, w_R) = (s_r, s_l), dw_L = dZ_m - dZ_r, dw_R = dZ_l - dZ_m
    (_dz_float64).  -> [3] float64 (h, f, w); with return_abs also [3] the sums of |A_0 dw_L| + |A_1 dw_R|."""
    landing = torch.as_tensor(landing, dtype=torch.float32)
    dev = landing.device
    tex = torch.as_tensor(tex, dtype=torch.float32, device=dev)
    gnum = torch.as_tensor(gnum, dtype=torch.float64, device=dev)
    x_tan = torch.as_tensor(x_tan, dtype=torch.float32, device=dev)
    L = len(inv_texels)
    if landing.shape[0] != 3 + 2 * L:
        raise ValueError(f"{L} layers need a landing record of {3 + 2 * L} rows and {L} inv_texels")
    if alpha is not None:
        alpha = torch.as_tensor(alpha, dtype=torch.float32, device=dev)
        if alpha.shape[0] != L:
            raise ValueError(f"alpha has {alpha.shape[0]} layers, inv_texels {L}")
    if x_tan.shape != landing.shape[1:]:
        raise ValueError(f"x_tan must be {tuple(landing.shape[1:])}, got {tuple(x_tan.shape)}")
    shared = tex.dim() == 3
    NT = int(tex.shape[-3])
    if tuple(gnum.shape) != (2, NT) + tuple(landing.shape[2:]):
        raise ValueError(f"gnum must be {(2, NT) + tuple(landing.shape[2:])}, got {tuple(gnum.shape)}")
    if gden is not None:
        gden = torch.as_tensor(gden, dtype=torch.float64, device=dev)
        if tuple(gden.shape) != (2,) + tuple(landing.shape[2:]):
            raise ValueError(f"gden must be {(2,) + tuple(landing.shape[2:])}, got {tuple(gden.shape)}")
    h, f, w, r = (float(v) for v in dp)
    ra = landing[0]
    live = ra != 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    T = torch.ones(ra.shape, dtype=torch.float64, device=dev)
    c = torch.zeros((NT,) + tuple(ra.shape), dtype=torch.float64, device=dev)
    for l in range(L):
        reads = live & (T != 0)                                 # the forward's walk ends where T reaches 0
        px, py = landing[3 + 2 * l], landing[4 + 2 * l]
        a = torch.ones_like(T) if alpha is None else _bilinear_float64(alpha[l:l + 1], px, py, inv_texels[l], reads)[0]
        t = _bilinear_float64(tex if shared else tex[l], px, py, inv_texels[l], reads)
        g = T * a
        c = torch.where(reads, c + g * t, c)
        T = torch.where(reads, T * (1 - a), T)
    A = []
    for side in range(2):
        s = gnum[side, 0] * c[0]
        for k in range(1, NT):
            s = s + gnum[side, k] * c[k]
        if gden is not None:
            s = s + gden[side]
        A.append(torch.where(live, ra.double() * s, zero))
    dZ = _dz_float64(x_tan.double(), h, f, w, r)                                             # [3, 3, S, H, W]
    dwl, dwr = dZ[1] - dZ[0], dZ[2] - dZ[1]
    used = live & ((A[0] != 0) | (A[1] != 0))
    grad = torch.where(used, A[0] * dwl + A[1] * dwr, zero).flatten(1).sum(1)
    if not return_abs:
        return grad
    return grad, torch.where(used, (A[0] * dwl).abs() + (A[1] * dwr).abs(), zero).flatten(1).sum(1)


def layer_dp_grad_batch(lens, alpha, tex, depths, inv_texels, x2, y2, trips, gnum, gden, dp, wvln=DEFAULT_WAVE,
                        pixel_center=True, x_tan=False):
    """ONE call of sdirt_render_layers_dp_grad: the counterpart of layer_batch (same scene, pupil points, dp, wvln and
    pixel_center), with `trips` the table that call ended with, gnum [2, T, H, W] float64 the adjoint of its num and
    gden [2, H, W] float64 the adjoint of its den, or None.  alpha=None: every layer opaque (render_plane's scene with
    L = 1).  -> [3] float64 on the lens's device: the gradient in (h, f, w), the entry's partial rows
    [ceil(T / 4), ceil(H W / 256), 3] added by one .sum over that fixed layout -- the same bits on every run;
    x_tan=True: -> (that, x_tan [S, H, W] fp32: the kernel's x_tan of every ray)."""
    dev = lens.device
    if dp is None:
        raise ValueError("dp=None: one view with unit weights has no sub-pixel model to differentiate")
    if alpha is None:
        if not torch.is_tensor(tex) or tex.dim() not in (3, 4) or tex.dtype != torch.float32:
            raise ValueError("the layers' image must be a float32 [L, C, Ht, Wt] tensor, or [C, Ht, Wt] shared by all layers")
        shared = tex.dim() == 3
        L, (T, Ht, Wt) = len(depths), (int(v) for v in tex.shape[-3:])
        if not 1 <= L <= _lib.MAX_LAYERS or len(inv_texels) != L or (not shared and int(tex.shape[0]) != L):
            raise ValueError(f"{L} depths, {len(inv_texels)} scales and an image of {tuple(tex.shape)}: layers differ")
    else:
        L, T, Ht, Wt, shared = _check_layers(alpha, tex, depths, inv_texels, scan=False)
        if alpha.device != dev:
            raise ValueError("alpha and tex must be on the lens's device")
        alpha = alpha.contiguous()
    if tex.device != dev:
        raise ValueError("alpha and tex must be on the lens's device")
    h, f, w, r = (float(v) for v in dp)
    if not r > 0 or f == h:
        raise ValueError("dp: r must be > 0 and f must differ from h")
    H, W = (int(v) for v in lens.sensor_res)
    S = int(x2.shape[0])
    K = len(lens.surfaces)
    if tuple(x2.shape) != (S, H, W) or tuple(y2.shape) != (S, H, W):
        raise ValueError(f"pupil points must be [spp, {H}, {W}], got {tuple(x2.shape)} and {tuple(y2.shape)}")
    if len(trips) != K:
        raise ValueError(f"{len(trips)} trip counts for a lens of {K} surfaces")
    if not torch.is_tensor(gnum) or gnum.dtype != torch.float64 or gnum.device != dev or tuple(gnum.shape) != (2, T, H, W):
        raise ValueError(f"gnum must be float64 {(2, T, H, W)} on the lens's device")
    if gden is not None and (not torch.is_tensor(gden) or gden.dtype != torch.float64 or gden.device != dev
                             or tuple(gden.shape) != (2, H, W)):
        raise ValueError(f"gden must be float64 {(2, H, W)} on the lens's device, or None")
    lens._require_gpu()
    x1, y1 = sensor_axes(lens, pixel_center)
    x2 = x2.to(dev, torch.float32).contiguous()
    y2 = y2.to(dev, torch.float32).contiguous()
    tex, gnum = tex.contiguous(), gnum.contiguous()
    gden = None if gden is None else gden.contiguous()
    partial = torch.empty(((T + 3) // 4, (H * W + 255) // 256, 3), dtype=torch.float64, device=dev)
    xt = torch.empty((S, H, W), dtype=torch.float32, device=dev) if x_tan else None
    dpp = C.byref(_lib.DpParams(h, f, w, r))
    z = (C.c_double * L)(*(float(d) for d in depths))
    inv = (C.c_double * L)(*(float(v) for v in inv_texels))
    pupilz, _ = lens.exit_pupil()
    wv = float(wvln if wvln < 10 else wvln * 1e-3)
    with lens._timed("render_layers_dp_grad"):
        _lib.check(_lib.lib().sdirt_render_layers_dp_grad(
            lens.dev_lens(wv), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
            float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), S, H, W, dpp, L, z, inv, dptr(alpha), dptr(tex),
            0 if shared else T * Ht * Wt, T, Ht, Wt, dptr(gnum), dptr(gden), dptr(partial), dptr(xt), stream_ptr(dev)))
    grad = partial.view(-1, 3).sum(0)
    return (grad, xt) if x_tan else grad


# ------------------------------------------------------------------------------------ gradients in the depths
def _tap_slopes(planes, idx, fu, fv, live, magnitudes=False):
    """d/dfu and d/dfv of _read_taps(planes, ...) from the four taps it reads -> two [N, S, H, W] float64 (0 on dead
    rays): (1 - fv)(v01 - v00) + fv (v11 - v10) and (1 - fu)(v10 - v00) + fu (v11 - v01).  Two taps that replicate
    addressing puts on one texel differ by an exact 0.  magnitudes: the same with |v01 - v00|, ... (no cancellation)."""
    t64 = planes.double().flatten(1)
    v00, v01, v10, v11 = (t64[:, idx[j]] for j in range(4))
    top, bottom, left, right = v01 - v00, v11 - v10, v10 - v00, v11 - v01
    if magnitudes:
        top, bottom, left, right = top.abs(), bottom.abs(), left.abs(), right.abs()
    zero = torch.zeros((), dtype=torch.float64, device=idx.device)
    return (torch.where(live, (1 - fv) * top + fv * bottom, zero), torch.where(live, (1 - fu) * left + fu * right, zero))


def layer_depth_grads_float64(landing, ray_dir, alpha, tex, inv_texels, gnum, return_abs=False):
    """The adjoint of DESIGN.md §7s from the forward's landing record and the backward's ray_dir record, in plain torch
    and without autograd: what sdirt_render_layers_depth_grad's partial rows add up to.

    landing, alpha (None: every layer opaque -- the ray meets layer 0 only), tex, inv_texels as in layer_sums_float64;
    ray_dir [3, S, H, W] fp32: dx, dy, dz of every ray as the trace left it; gnum [V, T, H, W] float64 (V = 1: one
    view from row 1 of landing, V = 2: rows 1 and 2).
    Per live ray: sx = dx / dz, sy = dy / dz; q_k, T_l, a_l, g_l, D_l, R_l, e_l of layer_grads_float64; every lookup's
    derivative from its four taps (_tap_slopes); Pu_l = e_l da_l/dfu + g_l sum_k q_k dt_{l,k}/dfu, Pv_l alike;
    gz_l = inv_l (Pv_l sy - Pu_l sx), ginv_l = Pv_l py_l - Pu_l px_l; layers with T_l == 0 give nothing.
    -> [L, 2] float64: the gradient in depths[l] and in inv_texels[l]; with return_abs also [L, 2] the sums of |term|,
    absolute values taken before any cancellation: |Pu|_l = T_l (Dbar_l + Rbar_{l+1}) |da/dfu| + g_l sum_k |q|_k
    |dt_k/dfu| with |d./dfu| = (1 - fv)|v01 - v00| + fv |v11 - v10|, |gz| = inv (|Pv| |sy| + |Pu| |sx|), |ginv| alike."""
    landing = torch.as_tensor(landing, dtype=torch.float32)
    dev = landing.device
    tex = torch.as_tensor(tex, dtype=torch.float32, device=dev)
    gnum = torch.as_tensor(gnum, dtype=torch.float64, device=dev)
    ray_dir = torch.as_tensor(ray_dir, dtype=torch.float32, device=dev)
    L = len(inv_texels)
    if landing.shape[0] != 3 + 2 * L:
        raise ValueError(f"{L} layers need a landing record of {3 + 2 * L} rows and {L} inv_texels")
    opaque = alpha is None
    if not opaque:
        alpha = torch.as_tensor(alpha, dtype=torch.float32, device=dev)
        if alpha.shape[0] != L:
            raise ValueError(f"alpha has {alpha.shape[0]} layers, inv_texels {L}")
    if tuple(ray_dir.shape) != (3,) + tuple(landing.shape[1:]):
        raise ValueError(f"ray_dir must be {(3,) + tuple(landing.shape[1:])}, got {tuple(ray_dir.shape)}")
    shared = tex.dim() == 3
    NT, Ht, Wt = (int(v) for v in tex.shape[-3:])
    V = int(gnum.shape[0]) if gnum.dim() == 4 else 0
    if V not in (1, 2) or tuple(gnum.shape) != (V, NT) + tuple(landing.shape[2:]):
        raise ValueError(f"gnum must be {('V', NT) + tuple(landing.shape[2:])} with V = 1 or 2, got {tuple(gnum.shape)}")
    ra = landing[0]
    live = ra != 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    dz = torch.where(live, ray_dir[2].double(), torch.ones((), dtype=torch.float64, device=dev))
    sx = torch.where(live, ray_dir[0].double() / dz, zero)
    sy = torch.where(live, ray_dir[1].double() / dz, zero)
    wr = torch.where(live, landing[1:1 + V].double() * ra.double(), zero)                   # [V, S, H, W]
    q = wr[0] * gnum[0][:, None]                                                            # [T, S, H, W]
    qa = wr[0] * gnum[0].abs()[:, None]
    if V == 2:
        q, qa = q + wr[1] * gnum[1][:, None], qa + wr[1] * gnum[1].abs()[:, None]
    T = torch.ones(ra.shape, dtype=torch.float64, device=dev)
    kept = []
    for l in range(1 if opaque else L):                         # an opaque layer 0 leaves T = 0: nothing behind it is read
        idx, w, fu, fv = _taps_float64(landing[3 + 2 * l], landing[4 + 2 * l], inv_texels[l], live, Ht, Wt, fractions=True)
        a = torch.ones_like(T) if opaque else _read_taps(alpha[l:l + 1], idx, w, live)[0]
        t = _read_taps(tex if shared else tex[l], idx, w, live)
        D, Dbar = q[0] * t[0], qa[0] * t[0].abs()
        for k in range(1, NT):
            D, Dbar = D + q[k] * t[k], Dbar + qa[k] * t[k].abs()
        kept.append((idx, fu, fv, a, D, Dbar, T))
        T = T * (1 - a)
    grad = torch.zeros((L, 2), dtype=torch.float64, device=dev)
    mags = torch.zeros((L, 2), dtype=torch.float64, device=dev)
    R, Rbar = torch.zeros_like(T), torch.zeros_like(T)
    for l in range(len(kept) - 1, -1, -1):
        idx, fu, fv, a, D, Dbar, Tl = kept[l]
        d = D - R
        sel = live & (Tl != 0)
        planes = tex if shared else tex[l]
        tu, tv = _tap_slopes(planes, idx, fu, fv, live)
        tua, tva = _tap_slopes(planes, idx, fu, fv, live, magnitudes=True)
        Cu, Cv, Cua, Cva = q[0] * tu[0], q[0] * tv[0], qa[0] * tua[0], qa[0] * tva[0]
        for k in range(1, NT):
            Cu, Cv, Cua, Cva = Cu + q[k] * tu[k], Cv + q[k] * tv[k], Cua + qa[k] * tua[k], Cva + qa[k] * tva[k]
        if opaque:
            au = av = aua = ava = torch.zeros_like(T)
        else:
            (au,), (av,) = _tap_slopes(alpha[l:l + 1], idx, fu, fv, live)
            (aua,), (ava,) = _tap_slopes(alpha[l:l + 1], idx, fu, fv, live, magnitudes=True)
        e, g, eb = Tl * d, Tl * a, Tl * (Dbar + Rbar)
        Pu, Pv = e * au + g * Cu, e * av + g * Cv
        Pua, Pva = eb * aua + g * Cua, eb * ava + g * Cva
        inv = float(np.float32(inv_texels[l]))
        px, py = landing[3 + 2 * l].double(), landing[4 + 2 * l].double()
        grad[l, 0] = torch.where(sel, inv * (Pv * sy - Pu * sx), zero).sum()
        grad[l, 1] = torch.where(sel, Pv * py - Pu * px, zero).sum()
        mags[l, 0] = torch.where(sel, inv * (Pva * sy.abs() + Pua * sx.abs()), zero).sum()
        mags[l, 1] = torch.where(sel, Pva * py.abs() + Pua * px.abs(), zero).sum()
        R, Rbar = R + a * d, a * Dbar + (1 - a) * Rbar
    return (grad, mags) if return_abs else grad


def layer_depth_grad_batch(lens, alpha, tex, depths, inv_texels, x2, y2, trips, gnum, dp=None, wvln=DEFAULT_WAVE,
                           pixel_center=True, ray_dir=False):
    """ONE call of sdirt_render_layers_depth_grad: the counterpart of layer_batch (same scene, pupil points, dp, wvln
    and pixel_center), with `trips` the table that call ended with and gnum [V, T, H, W] float64 the adjoint of its num.
    alpha=None: every layer opaque (render_plane's scene with L = 1).  -> [L, 2] float64 on the lens's device: the
    gradient in depths[l] and in inv_texels[l], the entry's partial rows [ceil(T / 4), ceil(H W / 256), L, 2] added by
    one .sum over that fixed layout -- the same bits on every run; ray_dir=True: -> (that, ray_dir [3, S, H, W] fp32:
    dx, dy, dz of every ray as the trace left it)."""
    dev = lens.device
    if alpha is None:
        if not torch.is_tensor(tex) or tex.dim() not in (3, 4) or tex.dtype != torch.float32:
            raise ValueError("the layers' image must be a float32 [L, C, Ht, Wt] tensor, or [C, Ht, Wt] shared by all layers")
        shared = tex.dim() == 3
        L, (T, Ht, Wt) = len(depths), (int(v) for v in tex.shape[-3:])
        if not 1 <= L <= _lib.MAX_LAYERS or len(inv_texels) != L or (not shared and int(tex.shape[0]) != L):
            raise ValueError(f"{L} depths, {len(inv_texels)} scales and an image of {tuple(tex.shape)}: layers differ")
    else:
        L, T, Ht, Wt, shared = _check_layers(alpha, tex, depths, inv_texels, scan=False)
        if alpha.device != dev:
            raise ValueError("alpha and tex must be on the lens's device")
        alpha = alpha.contiguous()
    if tex.device != dev:
        raise ValueError("alpha and tex must be on the lens's device")
    H, W = (int(v) for v in lens.sensor_res)
    S = int(x2.shape[0])
    K = len(lens.surfaces)
    V = 1 if dp is None else 2
    if tuple(x2.shape) != (S, H, W) or tuple(y2.shape) != (S, H, W):
        raise ValueError(f"pupil points must be [spp, {H}, {W}], got {tuple(x2.shape)} and {tuple(y2.shape)}")
    if len(trips) != K:
        raise ValueError(f"{len(trips)} trip counts for a lens of {K} surfaces")
    if not torch.is_tensor(gnum) or gnum.dtype != torch.float64 or gnum.device != dev or tuple(gnum.shape) != (V, T, H, W):
        raise ValueError(f"gnum must be float64 {(V, T, H, W)} on the lens's device")
    lens._require_gpu()
    x1, y1 = sensor_axes(lens, pixel_center)
    x2 = x2.to(dev, torch.float32).contiguous()
    y2 = y2.to(dev, torch.float32).contiguous()
    tex, gnum = tex.contiguous(), gnum.contiguous()
    partial = torch.empty(((T + 3) // 4, (H * W + 255) // 256, L, 2), dtype=torch.float64, device=dev)
    rd = torch.empty((3, S, H, W), dtype=torch.float32, device=dev) if ray_dir else None
    dpp = None if dp is None else C.byref(_lib.DpParams(*(float(v) for v in dp)))
    z = (C.c_double * L)(*(float(d) for d in depths))
    inv = (C.c_double * L)(*(float(v) for v in inv_texels))
    pupilz, _ = lens.exit_pupil()
    wv = float(wvln if wvln < 10 else wvln * 1e-3)
    with lens._timed("render_layers_depth_grad"):
        _lib.check(_lib.lib().sdirt_render_layers_depth_grad(
            lens.dev_lens(wv), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
            float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), S, H, W, dpp, L, z, inv, dptr(alpha), dptr(tex),
            0 if shared else T * Ht * Wt, T, Ht, Wt, dptr(gnum), dptr(partial), dptr(rd), stream_ptr(dev)))
    grad = partial.view(-1, L, 2).sum(0)
    return (grad, rd) if ray_dir else grad


def _depth_leaves(depths, scales, depth_grad):
    """The tensors among a call's depths and scales that get a gradient from a depth_grad=True call: -> (depths,
    scales), None where the argument is no tensor or requires none; both None without depth_grad or outside grad mode."""
    if not depth_grad or not torch.is_grad_enabled():
        return (None, None)
    return tuple(v if torch.is_tensor(v) and v.requires_grad else None for v in (depths, scales))


def _as_floats(v):
    """A call's depths or scales as the forward takes them: floats (a list of them; a 0-d tensor or a number: one)."""
    if v is None:
        return None
    if torch.is_tensor(v):
        v = v.detach().double().tolist()
    return float(v) if np.isscalar(v) else [float(x) for x in v]


def _dp_leaves(dp, dp_grad):
    """The tensors among dp's h, f, w that get a gradient from a dp_grad=True call: -> (h, f, w) with None where the
    entry is no tensor or requires none; all None without dp_grad, outside grad mode, or without such a tensor."""
    if not dp_grad:
        return (None, None, None)
    if dp is None:
        raise ValueError("dp_grad=True with dp=None: one view with unit weights has no sub-pixel model")
    if not torch.is_grad_enabled():
        return (None, None, None)
    return tuple(v if torch.is_tensor(v) and v.requires_grad else None for v in tuple(dp)[:3])


class _RenderRecorded(torch.autograd.Function):
    """render_plane / render_layers(scene_grad=True, dp_grad=True and / or depth_grad=True) under autograd.  The forward is the plain
    call (the same launches, the same images in every bit), which also keeps, per chunk of samples and wavelength
    group, the pupil points x2, y2 -- 8 bytes per ray, the only record that grows with the sample count -- and the trip
    table the launch ended with, and per call the wavelengths, pixel_center, dp, the depths, the inv_texels and the
    TOTAL den and num of every group.  The backward forms gnum = G / den_total (gnum_from_image_grad) once per
    wavelength group and runs over every recorded chunk
      sdirt_render_layers_grad into zeroed float64 buffers of the inputs' shapes, where img or alpha
      takes a gradient, and
      sdirt_render_layers_dp_grad with gden = gden_from_image_grad, where h, f or w does: the chunks'
      and the groups' [3] are added in the order recorded, and
      sdirt_render_layers_depth_grad, where `depths` or `scales` (1-D tensors of L; 0-d for
      render_plane) does: the [L, 2] are added in the order recorded, `depths` gets gdepth and `scales` gets
      ginv_texel_l (-inv_texel_l / scale_l);
    and returns them in the inputs' dtype (h, f, w, depths, scales: on their device).  It traces through the lens AS IT STANDS THEN: a
    lens changed (surfaces, sensor, focus, precision) between forward and backward is the caller's error."""

    @staticmethod
    def forward(ctx, img, alpha, lens, run, args, h=None, f=None, w=None, depths=None, scales=None):
        record = {"chunks": []}
        with torch.no_grad():
            res = run(lens, img, alpha, *args, record=record)
        res = res if isinstance(res, tuple) else (res,)
        ctx.lens, ctx.record = lens, record
        ctx.dp_leaves = tuple((v.dtype, v.device) if v is not None else None for v in (h, f, w))
        ctx.depth_leaves = tuple((v.dtype, v.device, v.shape) if v is not None else None for v in (depths, scales))
        ctx.save_for_backward(img, *(() if alpha is None else (alpha,)))
        ctx.set_materialize_grads(False)
        return res

    @staticmethod
    def backward(ctx, *G):
        lens, rec = ctx.lens, ctx.record
        img, alpha = (ctx.saved_tensors + (None,))[:2]
        need_img, need_alpha = ctx.needs_input_grad[0], alpha is not None and ctx.needs_input_grad[1]
        need_dp = [leaf is not None and need for leaf, need in zip(ctx.dp_leaves, ctx.needs_input_grad[5:8])]
        need_z = [leaf is not None and need for leaf, need in zip(ctx.depth_leaves, ctx.needs_input_grad[8:10])]
        none = (None,) * 10
        if all(g is None for g in G) or not (need_img or need_alpha or any(need_dp) or any(need_z)):
            return none
        shape = next(g.shape for g in G if g is not None)
        G = torch.stack([torch.zeros(shape, dtype=torch.float64, device=lens.device) if g is None else g.double()
                         for g in G])                                     # [V, (B,) C, H, W]
        H, W = (int(v) for v in shape[-2:])
        Ht, Wt = (int(v) for v in img.shape[-2:])
        V, chroma, plane = G.shape[0], rec["chroma"], rec["plane"]
        scene = need_img or need_alpha
        with torch.no_grad():
            gimg = torch.zeros(img.shape, dtype=torch.float64, device=lens.device) if need_img else None
            galpha = torch.zeros(alpha.shape, dtype=torch.float64, device=lens.device) if need_alpha else None
            # per wavelength group: the forward's planes, their image adjoint, and the buffer their gradient is added to
            if not chroma:
                texs = [img.detach().reshape(-1, Ht, Wt) if plane else img.detach()]
                Gs = [G.reshape(V, -1, H, W)]
                gtexs = [(gimg.view(-1, Ht, Wt) if plane else gimg) if need_img else None]
            else:
                texs, Gs, gtexs = [], [], []
                for c in range(len(rec["wv"])):
                    ch = img.detach()[:, c] if plane else (img.detach()[c:c + 1] if img.dim() == 3 else img.detach()[:, c:c + 1])
                    texs.append(ch.contiguous())
                    Gs.append(G[:, :, c] if plane else G[:, c:c + 1])
                    gtexs.append(torch.zeros(texs[-1].shape, dtype=torch.float64, device=lens.device) if need_img else None)
            gnums = [gnum_from_image_grad(Gg, rec["den"][g], rec["spp"], rec["photometric"]).contiguous()
                     for g, Gg in enumerate(Gs)]
            if any(need_dp):
                gdens = [gden_from_image_grad(Gg, rec["num"][g], rec["den"][g], rec["photometric"]) for g, Gg in enumerate(Gs)]
                gdp = torch.zeros(3, dtype=torch.float64, device=lens.device)
            if any(need_z):
                gz = torch.zeros((len(rec["depths"]), 2), dtype=torch.float64, device=lens.device)
            stack = None if plane else alpha.detach()
            for g, x2, y2, trips in rec["chunks"]:
                if scene:
                    layer_grad_batch(lens, stack, texs[g], rec["depths"], rec["inv_texels"], x2, y2, trips, gnums[g],
                                     rec["dp"], rec["wv"][g], rec["pixel_center"],
                                     galpha=galpha if need_alpha else False, gtex=gtexs[g] if need_img else False)
                if any(need_dp):
                    gdp += layer_dp_grad_batch(lens, stack, texs[g], rec["depths"], rec["inv_texels"], x2, y2, trips,
                                               gnums[g], gdens[g], rec["dp"], rec["wv"][g], rec["pixel_center"])
                if any(need_z):
                    gz += layer_depth_grad_batch(lens, stack, texs[g], rec["depths"], rec["inv_texels"], x2, y2, trips,
                                                 gnums[g], rec["dp"], rec["wv"][g], rec["pixel_center"])
            if chroma and need_img:
                for c, gt in enumerate(gtexs):
                    if plane:
                        gimg[:, c] = gt
                    elif img.dim() == 3:
                        gimg[c:c + 1] = gt
                    else:
                        gimg[:, c:c + 1] = gt
            gleaf = [gdp[j].to(device=leaf[1], dtype=leaf[0]) if need else None
                     for j, (leaf, need) in enumerate(zip(ctx.dp_leaves, need_dp))]
            gzs = [None, None]
            if any(need_z):
                # inv_texel = 1 / (scale pixel_size W / Wt): d inv_texel / d scale = -inv_texel / scale
                chain = torch.tensor([-v / s for v, s in zip(rec["inv_texels"], rec["scales"])], dtype=torch.float64,
                                     device=lens.device)
                for j, vals in enumerate((gz[:, 0], gz[:, 1] * chain)):
                    if need_z[j]:
                        dtype, device, shape = ctx.depth_leaves[j]
                        gzs[j] = vals.reshape(shape).to(device=device, dtype=dtype)
        return (gimg.to(img.dtype) if need_img else None, galpha.to(alpha.dtype) if need_alpha else None,
                None, None, None, *gleaf, *gzs)


def _recorded_call(lens, img, alpha, run, args, scene, leaves, zleaves=(None, None)):
    """The call through _RenderRecorded: img and alpha take part in the record only where scene_grad recorded them
    (a dp_grad=True call alone leaves them without a gradient, whatever they require), h, f, w where dp_grad did, the
    depths and the scales where depth_grad did; the forward runs with dp, the depths and the scales as floats."""
    dp = args[2]
    floats = None if dp is None else tuple(float(v.detach()) if torch.is_tensor(v) else float(v) for v in dp)
    args = (_as_floats(args[0]), args[1], floats, args[3], _as_floats(args[4])) + args[5:]
    if not scene:
        img, alpha = img.detach(), None if alpha is None else alpha.detach()
    return _RenderRecorded.apply(img, alpha, lens, run, args, *leaves, *zleaves)


def render_single_img(lens, img_org, depth=DEPTH, spp=64, unwarp=False, save_name=None, return_tensor=False, noise=0,
                      method="psf"):
    """optics.py:725-809: render one uint8 RGB ndarray [H, W, 3] for inspection, on a sensor of the image's resolution
    (the lens's own sensor is put back afterwards).  method='raytracing': render_plane at WAVE_RGB from
    sample_sensor's pixel corners with unit weights -- what the reference's undefined render_sample_ray /
    render_compute_image would have produced, upright without its flip; method='psf': psf_map(grid=21, ks=44) and
    render_psf_map.  Then the reference's noise, clamp and uint8 conversion (:792-809).  unwarp is undefined in the
    reference."""
    if not isinstance(img_org, np.ndarray):
        raise Exception("This function only supports ndarray input. If you want to render an image batch, use `render` "
                        "function.")
    if unwarp:
        raise NotImplementedError("unwarp: Lensgroup.unwarp is undefined in the reference")
    if method not in ("raytracing", "psf"):
        raise ValueError("method must be 'raytracing' or 'psf'")
    if len(img_org.shape) == 2:
        raise Exception("Monochrome image is not tested yet.")
    H, W, Cn = img_org.shape
    assert Cn == 3, "Only support RGB image, dtype should be ndarray."
    sensor = {k: getattr(lens, k) for k in ("sensor_res", "sensor_size", "pixel_size", "r_last")}
    try:
        lens.prepare_sensor(sensor_res=[H, W])                 # assigns before it asserts a square pixel: inside the try
        img = torch.tensor((img_org / 255.).astype(np.float32)).permute(2, 0, 1).unsqueeze(0).to(lens.device)
        if method == "raytracing":
            img_render = render_plane(lens, img, depth, spp=spp, dp=None, wvln=WAVE_RGB, pixel_center=False)
        else:
            from .render_psf import render_psf_map
            psf_grid, psf_ks = 21, 44
            img_render = render_psf_map(img, lens.psf_map(grid=psf_grid, ks=psf_ks, depth=depth), grid=psf_grid)
        if noise > 0:
            img_render = torch.clamp(img_render + torch.randn_like(img_render) * noise, 0, 1)
        if save_name is not None:
            # torchvision.utils.save_image of a one-image batch: clamped to [0, 1], rounded to 8 bits
            from .plots import _pyplot
            rgb = img_render[0].mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
            _pyplot().imsave(f"{save_name}.png", rgb)
    finally:
        for k, v in sensor.items():
            setattr(lens, k, v)
    if return_tensor:
        return img_render
    return img_render[0, ...].mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
