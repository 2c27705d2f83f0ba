"""Ray-traced dual-pixel rendering of a textured plane through the lens: the backward renderer the
reference names in render_single_img(method='raytracing') (deeplens/optics.py:756-780) and never defines.

The reference has the ray generator (sample_sensor, optics.py:497-538), the trace to object space (trace2obj,
:630-635) and the caller; `render_sample_ray` and `render_compute_image` do not exist there.  Here the whole per-ray
program -- sample a sensor-side ray, take its dual-pixel weights from the direction it arrives with, trace it backward
through every surface, carry it to the plane, read the texture, sum -- is ONE HIP kernel (sdirt_render_plane,
csrc/sdirt_render_rt.hip); this module is its host side, the reference's two samplers, `render_single_img`, and a
pure-torch float64 restatement of the lookup and the sums (`plane_sums_float64`) that tests and tools check it with.

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
    inv = torch.tensor(float(inv_texel), dtype=torch.float32, device=landing.device)
    u = Wt / 2 - px * inv                                    # fp32, one rounding per operation
    v = Ht / 2 + py * inv
    a, b = u - 0.5, v - 0.5
    c0, r0 = torch.floor(a), torch.floor(b)
    fu, fv = (a - c0).double(), (b - r0).double()
    live = ra != 0
    # dead rays land anywhere (NaN included) and contribute nothing: give them a texel to read, then leave them out
    c0 = torch.where(live, c0, torch.zeros_like(c0)).clamp(-2, Wt).nan_to_num(nan=0.0).long()
    r0 = torch.where(live, r0, torch.zeros_like(r0)).clamp(-2, Ht).nan_to_num(nan=0.0).long()
    cl, cr = c0.clamp(0, Wt - 1), (c0 + 1).clamp(0, Wt - 1)
    rt, rb = r0.clamp(0, Ht - 1), (r0 + 1).clamp(0, Ht - 1)
    t64 = tex.double()
    t = ((1 - fv) * (1 - fu)) * t64[:, rt, cl] + ((1 - fv) * fu) * t64[:, rt, cr] \
        + (fv * (1 - fu)) * t64[:, rb, cl] + (fv * fu) * t64[:, rb, cr]                     # [T, S, H, W]
    zero = torch.zeros((), dtype=torch.float64, device=landing.device)
    t = torch.where(live, t, zero)
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


@torch.no_grad()
def render_plane(lens, img, depth, spp=64, dp=None, wvln=DEFAULT_WAVE, scale=None, pixel_center=True,
                 photometric=False, pupil_points=None, return_sums=False):
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
    No gradients."""
    chroma = _check_render_arguments(lens, img, spp, wvln, pupil_points)
    lens._require_gpu()
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
