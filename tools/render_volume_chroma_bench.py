#!/usr/bin/env python3
"""Times of the render from a CHROMATIC PSF volume [C,Dz,Gy,Gx,2,ks,ks], fused against what could be written before it
existed, in one process:

    python3 tools/render_volume_chroma_bench.py --steps 20 --warmup 3

1 x 3 x 512 x 768, ks 21, volume 3 x 16 x 32 x 32, random depth per pixel, the same operands for both paths:

    fused      local_dp_psf_render_volume on the 7-D volume: ONE call of sdirt_render_psf_volume_chroma, and of
               sdirt_render_psf_volume_chroma_grad / _grad_scene for the three backwards
    composed   three calls of the achromatic entries at C = 1 on img[:, c:c+1].contiguous() and vol[c], the results
               concatenated (the slice copies and the concatenation are part of the path, and of its backward)

The volume traffic per channel is the same in both; the fused form saves the table reads, the weights, two launches
and the copies.  Device-event times around `steps` calls after `warmup` calls, the two paths alternating round by round
(--rounds), the median round reported; the backward times are those of backward() alone (the forward that builds the
graph is outside the events).  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdirt_amd.render_psf import local_dp_psf_render_volume                                          # noqa: E402


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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_volume_chroma_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    b, c, h, w, ks = 1, 3, a.height, a.width, a.ks
    dz, gy, gx = a.grid
    gen = torch.Generator(device=dev).manual_seed(0)
    mk = lambda *s: torch.rand(s, generator=gen, dtype=torch.float32, device=dev)
    img, vol, G, z = mk(b, c, h, w), mk(c, dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w), mk(b, h, w)
    xn = torch.linspace(-1 + 1 / (2 * gx), 1 - 1 / (2 * gx), gx, device=dev)
    yn = torch.linspace(1 - 1 / (2 * gy), -1 + 1 / (2 * gy), gy, device=dev)
    zn = torch.linspace(0, 1, dz, device=dev) ** 2 if dz > 1 else torch.zeros(1, device=dev)
    vol_leaf, img_leaf, z_leaf = (t.clone().requires_grad_(True) for t in (vol, img, z))

    def fused(im, v, zz, **kw):
        return local_dp_psf_render_volume(im, v, xn, yn, zn, zz, ks, **kw)

    def composed(im, v, zz, **kw):
        per = [local_dp_psf_render_volume(im[:, k:k + 1].contiguous(), v[k], xn, yn, zn, zz, ks, **kw) for k in range(c)]
        return torch.cat([r[:, :1] for r in per] + [r[:, 1:] for r in per], 1)

    def forward_of(render):
        def run(_):
            with torch.no_grad():
                return render(img, vol, z)
        return run

    def backward(out):
        vol_leaf.grad = img_leaf.grad = z_leaf.grad = None
        out.backward(G)

    paths = {}
    for name, render in (("fused", fused), ("composed", composed)):
        paths[f"{name}_forward"] = (forward_of(render), None)
        paths[f"{name}_backward"] = (backward, lambda r=render: r(img, vol_leaf, z))
        paths[f"{name}_backward_image"] = (backward, lambda r=render: r(img_leaf, vol, z, scene_grad=True))
        paths[f"{name}_backward_depth"] = (backward, lambda r=render: r(img, vol, z_leaf, scene_grad=True))
    order = [f"{name}_{stage}" for stage in ("forward", "backward", "backward_image", "backward_depth")
             for name in ("fused", "composed")]
    rounds = {name: [] for name in order}
    for _ in range(a.rounds):                                # the paths alternate: a drift of the clock hits both
        for name in order:
            fn, setup = paths[name]
            rounds[name].append(timed(fn, a.steps, a.warmup, setup))
    res = {"shape": [b, c, h, w, ks], "volume": [c, dz, gy, gx], "steps": a.steps, "rounds": a.rounds,
           "volume_bytes": 4 * vol.numel()}
    for name, us in rounds.items():
        res[name] = {"event_us_median": round(statistics.median(us), 1), "event_us_rounds": [round(u, 1) for u in us]}
    for stage in ("forward", "backward", "backward_image", "backward_depth"):
        res[f"composed_over_fused_{stage}"] = round(res[f"composed_{stage}"]["event_us_median"]
                                                    / res[f"fused_{stage}"]["event_us_median"], 2)
    res["outputs_bit_equal"] = bool(torch.equal(forward_of(fused)(None), forward_of(composed)(None)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
