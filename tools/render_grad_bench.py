#!/usr/bin/env python3
"""Times of the per-pixel convolution's backward kernels beside its forward, in one process:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python3 tools/render_grad_bench.py --steps 20 --warmup 3

512 x 768 RGB, ks 21, fp32 (half = 0), the same operands for the three calls: sdirt_local_psf_render (the yardstick:
it moves the same 1.39 GB of kernels and is unchanged code), sdirt_local_psf_render_grad_psf and
sdirt_local_psf_render_grad_img (two kernels: the tiles and the gather).  The kernel times are rocprofv3's
(*_kernel_stats.csv); the device-event times printed here include the launches and are a cross-check only.  One JSON
line: event times, the bytes each call has to move, and what that is of 8 TB/s.  HBM counters are collected in runs
of their own (--pmc FETCH_SIZE, --pmc WRITE_SIZE with --steps 2 --warmup 1)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdirt_amd import _lib                                   # noqa: E402
from sdirt_amd.basics import dptr, stream_ptr                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--ks", type=int, default=21)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_grad_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    b, c, h, w, ks = 1, 3, a.height, a.width, a.ks
    gen = torch.Generator(device=dev).manual_seed(0)
    mk = lambda *s: torch.rand(s, generator=gen, dtype=torch.float32, device=dev)
    img, psf, gl, gr = mk(b, c, h, w), mk(b, h, w, 2, ks, ks), mk(b, c, h, w), mk(b, c, h, w)
    out_l, out_r, dimg, dpsf = torch.empty_like(img), torch.empty_like(img), torch.empty_like(img), torch.empty_like(psf)
    lib, st = _lib.lib(), stream_ptr(dev)
    nbytes = lib.sdirt_local_psf_render_grad_img_workspace_bytes(b, c, h, w, ks)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    calls = {
        "forward": lambda: lib.sdirt_local_psf_render(dptr(img), dptr(psf), b, c, h, w, ks, 0, dptr(out_l), dptr(out_r), st),
        "grad_psf": lambda: lib.sdirt_local_psf_render_grad_psf(dptr(img), dptr(gl), dptr(gr), b, c, h, w, ks, dptr(dpsf), st),
        "grad_img": lambda: lib.sdirt_local_psf_render_grad_img(dptr(psf), dptr(gl), dptr(gr), b, c, h, w, ks, dptr(dimg),
                                                                dptr(work), nbytes, st),
    }
    image, kernels = 4 * b * c * h * w, 4 * b * h * w * 2 * ks * ks
    # what each call has to move: its large operand once, the small ones once; grad_img also writes and re-reads its partials
    algorithmic = {"forward": kernels + 3 * image, "grad_psf": kernels + 3 * image, "grad_img": kernels + 3 * image + 2 * nbytes}
    res = {"shape": [b, c, h, w, ks], "steps": a.steps, "workspace_bytes": nbytes}
    for name, call in calls.items():
        for _ in range(a.warmup):
            _lib.check(call())
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            _lib.check(call())
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.steps
        res[name] = {"event_us": round(us, 2), "algorithmic_bytes": algorithmic[name],
                     "frac_of_8TBs": round(algorithmic[name] / (us * 1e-6) / 8e12, 4)}
    res["grad_psf_over_forward"] = round(res["grad_psf"]["event_us"] / res["forward"]["event_us"], 3)
    res["grad_img_over_forward"] = round(res["grad_img"]["event_us"] / res["forward"]["event_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
