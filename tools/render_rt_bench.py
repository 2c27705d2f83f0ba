#!/usr/bin/env python3
"""One frame (512 x 768, RGB, 64 spp) of a textured plane behind rf50mm, rendered three ways:

  fused   Lensgroup.render_plane: the one kernel of csrc/sdirt_render_rt.hip;
  staged  the same rays through the kernels that existed before it -- sample_sensor's arithmetic (Ray), trace,
          propagate_to -- with the dual-pixel weights, the lookup and the sums in torch (render_rt.plane_sums_float64);
  psf     local_dp_psf_render with a psf_lr kernel pair of the same plane for every pixel (ks 21).

Written to profiles/render_rt/bench.json (and printed): the fused kernel's time (HIP events around its launches), the
staged chain's time on the same box, how far the fused sums are from the staged chain's, and the largest and the mean
absolute difference between the ray-traced and the PSF-rendered pair -- at 64 spp and again at 256 spp, so that the
Monte-Carlo share of that difference shows.  Measurements, no targets.

  python tools/render_rt_bench.py [--depth -1500] [--out profiles/render_rt/bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import make_lens  # noqa: E402

from sdirt_amd import local_dp_psf_render  # noqa: E402
from sdirt_amd.basics import Ray  # noqa: E402
from sdirt_amd.render_rt import images_from_sums, plane_sums_float64, sensor_axes  # noqa: E402

DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
WVLN = 0.589
KS = 21


def weights_torch(x_tan, h, f, w, r):
    """(sl, sr) of monte_carlo.py:170-203 (r <= 0.5) in fp32 torch, literally."""
    def seg(x):
        u = torch.arccos(torch.clamp(x, -r, r) / r)
        return u - 0.5 * torch.sin(2 * u)

    fx, fmh = f * x_tan, f - h
    xr, xm, xl = w - (fx - w) * h / fmh, -fx * h / fmh, -w - (fx + w) * h / fmh
    sr_ml, sl_ml = r * r * (seg(xm) - seg(xr)), r * r * (seg(xl) - seg(xm))
    xr, xm, xl = (torch.clamp(v, -0.5, 0.5) for v in (w - h * x_tan, -h * x_tan, -w - h * x_tan))
    sr_mg, sl_mg = (xr - xm) - r * r * (seg(xm) - seg(xr)), (xm - xl) - r * r * (seg(xl) - seg(xm))
    return sl_ml + sl_mg, sr_ml + sr_mg


def texture(H, W):
    """Smooth noise with a few hard edges, in [0, 1]."""
    g = torch.Generator().manual_seed(0)
    t = torch.nn.functional.interpolate(torch.rand(1, 3, H // 8, W // 8, generator=g), size=(H, W), mode="bilinear")
    t[..., H // 4:H // 4 + 6, :] = 1.0
    t[..., :, W // 3:W // 3 + 6] = 0.0
    return t.clamp(0, 1).to(DEV)


def staged_sums(lens, tex, depth, x2, y2, inv):
    x1, y1 = sensor_axes(lens, pixel_center=True)
    gx, gy = torch.meshgrid(x1, y1, indexing="xy")
    o = torch.stack((gx, gy, torch.full_like(gx, lens.d_sensor)), 2)
    o2 = torch.stack((x2, y2, torch.full_like(x2, lens.exit_pupil()[0])), -1)
    ray = Ray(torch.broadcast_to(o, o2.shape), o2 - o, wvln=WVLN, device=lens.device)
    n = ray.numel
    x_tan = (ray.soa[3, :n] / -ray.soa[5, :n]).view(ray.shape)
    sl, sr = weights_torch(x_tan, *DP)
    lens.trace2obj(ray, depth)
    land = torch.stack([ray.soa[0, :n].view(ray.shape), ray.soa[1, :n].view(ray.shape), ray.soa[6, :n].view(ray.shape), sr, sl])
    num = torch.empty((2, tex.shape[0]) + tuple(ray.shape[1:]), dtype=torch.float64, device=DEV)
    den = torch.empty((2,) + tuple(ray.shape[1:]), dtype=torch.float64, device=DEV)
    rows = 64                                                  # the float64 terms of 64 sensor rows at a time
    for r0 in range(0, ray.shape[1], rows):
        num[:, :, r0:r0 + rows], den[:, r0:r0 + rows] = plane_sums_float64(land[:, :, r0:r0 + rows], tex, inv)
    return num, den


def timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=float, default=-1500.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_rt", "bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lens = make_lens("rf50mm", DEV)
    torch.manual_seed(0)
    lens.refocus(-1000 + lens.d_sensor)
    lens.prepare_sensor(sensor_res=(512, 768), sensor_size=(24.0, 36.0))
    H, W = lens.sensor_res
    depth = a.depth
    # the traced magnification: with it the ray-traced image registers with the texture as the PSF render does, whose
    # kernels are centred on their chief rays (the pinhole scale psf_lr lays its object points out with is recorded
    # beside it: a few per cent off, which only moves the field position a kernel is computed for)
    torch.manual_seed(3)
    scale = float(lens.calc_scale_ray(depth))
    inv = 1.0 / (scale * lens.pixel_size)
    img = texture(H, W)
    res = {"sensor": [H, W], "depth": depth, "scale_ray": scale, "scale_pinhole": float(lens.calc_scale_pinhole(depth)),
           "dp": DP, "wvln": WVLN, "ks": KS, "device": torch.cuda.get_device_name(0)}

    # the pupil points of 256 samples per pixel; the first 64 are the 64-spp frame
    torch.manual_seed(1)
    pz, pr = lens.exit_pupil()
    o2 = torch.cat([lens.sample_pupil((H, W), 64, pupilr=pr, pupilz=pz) for _ in range(4)])
    x2, y2 = o2[..., 0].contiguous(), o2[..., 1].contiguous()
    del o2

    def fused(spp):
        return lens.render_plane(img, depth, spp=spp, dp=DP, wvln=WVLN, scale=scale, pupil_points=(x2[:spp], y2[:spp]),
                                 return_sums=True)

    fused(64)                                                  # warm: the trip table is learnt, the lens uploaded
    lens.kernel_events = {}
    wall, (L, R, num, den) = timed(lambda: fused(64), a.reps)
    torch.cuda.synchronize()
    ev = [e0.elapsed_time(e1) for e0, e1 in lens.kernel_events["render_plane"]]
    lens.kernel_events = None
    res["fused_64spp"] = {"kernel_ms_median": float(np.median(ev)), "kernel_ms_all": [round(v, 3) for v in ev],
                          "launches_per_call": len(ev) / a.reps, "call_wall_ms_median": wall}

    staged_sums(lens, img[0], depth, x2[:64], y2[:64], inv)
    wall_s, (snum, sden) = timed(lambda: staged_sums(lens, img[0], depth, x2[:64], y2[:64], inv), a.reps)
    res["staged_64spp"] = {"wall_ms_median": wall_s}
    simg = images_from_sums(snum, sden)
    fimg = images_from_sums(num[:, 0], den)
    res["fused_vs_staged_64spp"] = {"max_abs": float((fimg - simg).abs().max()), "mean_abs": float((fimg - simg).abs().mean())}
    del snum, sden, simg, fimg

    # per-pixel psf_lr kernels of the same plane, then the per-pixel convolution
    gx, gy = torch.meshgrid(torch.linspace(-1, 1, W), torch.linspace(1, -1, H), indexing="xy")
    pts = torch.stack((gx, gy, torch.full_like(gx, depth)), -1).reshape(-1, 3)
    psf = torch.empty((H * W, 2, KS, KS), dtype=torch.float32, device=DEV)
    torch.manual_seed(2)
    t0 = time.perf_counter()
    step = 16384
    for n0 in range(0, H * W, step):
        lens.psf_lr(pts[n0:n0 + step], ks=KS, wvln=WVLN, dp=DP, normalize=False, out=psf[n0:n0 + step])
    psf /= psf.sum((-1, -2), keepdim=True).clamp_min(1e-30)    # every kernel sums to one, as num / den normalises a pixel
    torch.cuda.synchronize()
    res["psf_lr_all_pixels_s"] = time.perf_counter() - t0
    lr = local_dp_psf_render(img, psf.view(1, H, W, 2, KS, KS), kernel_size=KS)
    PL, PR = lr[:, :3], lr[:, 3:]
    del psf

    def against_psf(L, R):
        d = torch.stack((L - PL, R - PR)).abs()
        inner = d[..., KS:-KS, KS:-KS]                         # away from the frame, where the convolution pads
        return {"max_abs": float(d.max()), "mean_abs": float(d.mean()),
                "max_abs_inner": float(inner.max()), "mean_abs_inner": float(inner.mean())}

    res["raytraced_vs_psf_64spp"] = against_psf(L, R)
    L4, R4, _, _ = fused(256)
    res["raytraced_vs_psf_256spp"] = against_psf(L4, R4)
    res["raytraced_64_vs_256spp"] = {"max_abs": float(torch.stack((L - L4, R - R4)).abs().max()),
                                     "mean_abs": float(torch.stack((L - L4, R - R4)).abs().mean())}
    res["left_right_mean_abs"] = {"raytraced_256spp": float((L4 - R4).abs().mean()), "psf": float((PL - PR).abs().mean())}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
