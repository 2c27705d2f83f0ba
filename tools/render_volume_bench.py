#!/usr/bin/env python3
"""Times of the render from a PSF volume, fused against composed, in one process:

    python3 tools/render_volume_bench.py --steps 20 --warmup 3
    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python3 tools/render_volume_bench.py --steps 5 --warmup 2 --fused-only

1 x 3 x 512 x 768, ks 21, volume 16 x 32 x 32, random depth per pixel (every pixel in another depth segment), the same
operands for both paths:

    fused      local_dp_psf_render_volume (sdirt_render_psf_volume) and its backward (sdirt_render_psf_volume_grad)
    composed   the per-pixel kernels [B,H,W,2,ks,ks] (1.39 GB) interpolated with torch ops from the same segment tables,
               then local_dp_psf_render, and torch autograd through both for the backward
    scene      scene_grad=True: the backward in the image alone and in the depth alone
               (sdirt_render_psf_volume_grad_scene with the other output NULL), against the composed path's -- the
               image through local_dp_psf_render's backward on the materialised kernels, the depth back through the
               materialisation (torch autograd through the interpolation weights and axis_segments)

Device-event times around `steps` calls after `warmup` calls, the two paths alternating round by round (--rounds), the
median round reported; the backward times are those of backward() alone (the forward that builds the graph is outside
the events).  The kernel times proper are rocprofv3's, from a run of their own.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdirt_amd.render_psf import (axis_segments, local_dp_psf_render, local_dp_psf_render_volume,      # noqa: E402
                                  volume_segment_tables)


def interpolate_kernels(vol, tables):
    """The per-pixel kernels [B,H,W,2,ks,ks] from V with torch ops: the sum over the 8 corners of w * V[corner]."""
    ix, fx, iy, fy, iz, fz = tables
    dz, gy, gx = vol.shape[:3]
    ends = lambda i, f, n: ((i.long().clamp(0, max(n - 2, 0)), 1 - f), ((i.long().clamp(0, max(n - 2, 0)) + 1).clamp(max=n - 1), f))
    out = 0
    for zi, wz in ends(iz, fz, dz):
        for yi, wy in ends(iy, fy, gy):
            for xi, wx in ends(ix, fx, gx):
                w = (wz * wy.reshape(1, -1, 1)) * wx.reshape(1, 1, -1)
                out = out + w[..., None, None, None] * vol[zi, yi.reshape(1, -1, 1), xi.reshape(1, 1, -1)]
    return out


def timed(fn, steps, warmup, setup=None):
    for _ in range(warmup):
        fn(setup() if setup else None)
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(steps):
        arg = setup() if setup else None
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn(arg)
        t1.record()
        torch.cuda.synchronize()
        total += t0.elapsed_time(t1)
    return total * 1e3 / steps                               # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--ks", type=int, default=21)
    ap.add_argument("--grid", type=int, nargs=3, default=[16, 32, 32], metavar=("DZ", "GY", "GX"))
    ap.add_argument("--fused-only", action="store_true", help="for a profiler run: the HIP kernels alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_volume_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    b, c, h, w, ks = 1, 3, a.height, a.width, a.ks
    dz, gy, gx = a.grid
    gen = torch.Generator(device=dev).manual_seed(0)
    mk = lambda *s: torch.rand(s, generator=gen, dtype=torch.float32, device=dev)
    img, vol, G, z = mk(b, c, h, w), mk(dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w), mk(b, h, w)
    xn = torch.linspace(-1 + 1 / (2 * gx), 1 - 1 / (2 * gx), gx, device=dev)
    yn = torch.linspace(1 - 1 / (2 * gy), -1 + 1 / (2 * gy), gy, device=dev)
    zn = torch.linspace(0, 1, dz, device=dev) ** 2 if dz > 1 else torch.zeros(1, device=dev)
    tables = volume_segment_tables(xn, yn, zn, z, h, w)
    leaf = vol.clone().requires_grad_(True)

    def fused_forward(_):
        with torch.no_grad():
            return local_dp_psf_render_volume(img, vol, xn, yn, zn, z, ks)

    def composed_forward(_):
        with torch.no_grad():
            return local_dp_psf_render(img, interpolate_kernels(vol, tables), ks)

    img_leaf, z_leaf = img.clone().requires_grad_(True), z.clone().requires_grad_(True)

    def backward(out):
        leaf.grad = img_leaf.grad = z_leaf.grad = None
        out.backward(G)

    def composed_in_depth():
        iz, fz = axis_segments(zn, z_leaf)
        return local_dp_psf_render(img, interpolate_kernels(vol, (*tables[:4], iz, fz)), ks)

    paths = {
        "fused_forward": (fused_forward, None),
        "fused_backward": (backward, lambda: local_dp_psf_render_volume(img, leaf, xn, yn, zn, z, ks)),
        "composed_forward": (composed_forward, None),
        "composed_backward": (backward, lambda: local_dp_psf_render(img, interpolate_kernels(leaf, tables), ks)),
        "fused_backward_image": (backward, lambda: local_dp_psf_render_volume(img_leaf, vol, xn, yn, zn, z, ks,
                                                                              scene_grad=True)),
        "composed_backward_image": (backward, lambda: local_dp_psf_render(img_leaf, interpolate_kernels(vol, tables), ks)),
        "fused_backward_depth": (backward, lambda: local_dp_psf_render_volume(img, vol, xn, yn, zn, z_leaf, ks,
                                                                              scene_grad=True)),
        "composed_backward_depth": (backward, composed_in_depth),
    }
    if a.fused_only:
        paths = {k: v for k, v in paths.items() if k.startswith("fused")}
    rounds = {name: [] for name in paths}
    for _ in range(a.rounds):                                # the paths alternate: a drift of the clock hits both
        for name, (fn, setup) in paths.items():
            rounds[name].append(timed(fn, a.steps, a.warmup, setup))
    res = {"shape": [b, c, h, w, ks], "volume": [dz, gy, gx], "steps": a.steps, "rounds": a.rounds,
           "per_pixel_kernel_bytes": 4 * b * h * w * 2 * ks * ks, "volume_bytes": 4 * vol.numel()}
    for name, us in rounds.items():
        res[name] = {"event_us_median": round(statistics.median(us), 1), "event_us_rounds": [round(u, 1) for u in us]}
    if not a.fused_only:
        for stage in ("forward", "backward", "backward_image", "backward_depth"):
            res[f"composed_over_fused_{stage}"] = round(res[f"composed_{stage}"]["event_us_median"]
                                                        / res[f"fused_{stage}"]["event_us_median"], 2)
        same = torch.allclose(fused_forward(None), composed_forward(None), rtol=0, atol=1e-3)
        res["outputs_agree_to_1e-3"] = bool(same)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
