#!/usr/bin/env python3
"""Time the splat backward kernel (sdirt_forward_integral_grad) on its own and report counted HBM bytes per second.

Two shapes: the staged shape (4096 points x 4096 samples, ks 65) and the calibration shape (64 points x 65536
samples, ks 21).  Synthetic sensor-plane rays (spread over the PSF window, |x_tan| < 0.3, every ray valid) and random
upstream gradients; the DP parameters are the reference's defaults with r = 0.5 (small-r model) unless --big.
Counted bytes: the five ray arrays the kernel reads (o.x, o.y, d.x, d.z, ra: 20 B per ray), the two upstream grids
(8 B per pixel, once per workgroup that stages them) and the float64 partials it stores.
--focus: the six-component entry instead (sdirt_forward_integral_grad_focus: the sensor position as well; it reads d.y
too, 24 B per ray, and stores six partials), on the same rays with d.y spread like d.x.  In a kernel trace both are
k_forward_integral_grad<BIG, M, STAGE, FOCUS>, FOCUS the last template argument.
--rays: the per-ray entry (sdirt_forward_integral_grad_rays with a null `partial`: k_forward_integral_grad_rays alone),
which stores ray_grad [4, M] fp32 (16 B per ray) and no partials.

Usage:  python tools/grad_bench.py [--iters 50] [--big] [--ieee] [--focus | --rays]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdirt_amd import _lib  # noqa: E402
from sdirt_amd.basics import Ray, dptr, stream_ptr  # noqa: E402

PS = 0.005


def bench(N, S, ks, iters, r, flags, focus=False, rays=False):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ray = Ray.empty((S, N), device=dev)
    half = (ks / 2 - 1) * PS
    M = S * N
    ray.soa[0, :M] = (torch.rand(M, device=dev, generator=g) * 2 - 1) * half
    ray.soa[1, :M] = (torch.rand(M, device=dev, generator=g) * 2 - 1) * half
    ray.soa[2, :M] = 0.0
    ray.soa[3, :M] = (torch.rand(M, device=dev, generator=g) * 2 - 1) * 0.3
    ray.soa[4, :M] = (torch.rand(M, device=dev, generator=g) * 2 - 1) * 0.3 if focus else 0.0
    ray.soa[5, :M] = 1.0
    ray.soa[6, :M] = 1.0
    center = torch.zeros((N, 2), dtype=torch.float32, device=dev)
    gl = torch.randn((N, ks, ks), device=dev, generator=g)
    gr = torch.randn((N, ks, ks), device=dev, generator=g)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    h = _lib.lib()
    ns = int(h.sdirt_forward_integral_grad_slices(N, S, ncu))
    comps = 6 if focus else 5
    partial = torch.empty((4, M), dtype=torch.float32, device=dev) if rays else \
        torch.empty((N, ns, comps), dtype=torch.float64, device=dev)
    dp = _lib.DpParams(0.78, 1.44, 0.3, r)
    entry = h.sdirt_forward_integral_grad_focus if focus else h.sdirt_forward_integral_grad

    def launch():
        if rays:
            _lib.check(h.sdirt_forward_integral_grad_rays(ray.c_rays(), S, N, PS, ks, dptr(center), C.byref(dp), flags,
                                                          dptr(gl), dptr(gr), None, ns, dptr(partial), stream_ptr(dev)))
        else:
            _lib.check(entry(ray.c_rays(), S, N, PS, ks, dptr(center), C.byref(dp), flags,
                             dptr(gl), dptr(gr), dptr(partial), ns, stream_ptr(dev)))
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    first = partial.clone()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / iters
    assert torch.equal(first, partial), "the backward kernel is not run-to-run identical"
    nbytes = (24 if focus else 20) * M + 8 * ks * ks * N * ns + (16 * M if rays else 8 * comps * N * ns)
    return dict(points=N, spp=S, ks=ks, slices=ns, ms=round(ms, 4), gbytes=round(nbytes / 1e9, 4),
                gb_per_s=round(nbytes / ms / 1e6, 1), frac_of_8tbs=round(nbytes / ms / 1e6 / 8000, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--big", action="store_true", help="r = 0.65 (big-r model)")
    ap.add_argument("--ieee", action="store_true", help="SDIRT_PSF_STRICT_IEEE")
    ap.add_argument("--focus", action="store_true", help="the six-component entry sdirt_forward_integral_grad_focus")
    ap.add_argument("--rays", action="store_true", help="the per-ray entry sdirt_forward_integral_grad_rays, partial = NULL")
    args = ap.parse_args()
    if args.focus and args.rays:
        ap.error("--focus and --rays are two entries: one at a time")
    r = 0.65 if args.big else 0.5
    flags = _lib.PSF_STRICT_IEEE if args.ieee else 0
    for N, S, ks in ((4096, 4096, 65), (64, 65536, 21)):
        res = bench(N, S, ks, args.iters, r, flags, args.focus, args.rays)
        res.update(r=r, precision="ieee" if args.ieee else "lean",
                   entry="focus" if args.focus else "rays" if args.rays else "grad")
        print(json.dumps(res))


if __name__ == "__main__":
    main()
