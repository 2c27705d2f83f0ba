#!/usr/bin/env python3
"""The layered render's backward into the layer depths (k_render_layers_depth_grad) measured on one
box, one run:

  512 x 768 RGB frame behind rf50mm, 64 spp, the three planes sharing one trace, default dp, on the scenes of
  tools/render_layers_bench.py: one opaque layer, and the `extend`ed RGB-D stacks of 4 and 8 layers.  Per scene the
  forward kernel (k_render_layers) and the new backward into the depths, and -- one opaque layer -- with a null alpha
  (render_plane's backward), HIP events around the launches.  All calls are warmed --warm times each and then timed in
  turn, round after round (a drift of the box falls on all alike); median and range of --reps rounds, and the ratio
  of every backward's median to the forward's of the same scene and run.

Written to profiles/render_depth_grad/bench.json (and printed).  Measurements, no targets: one scene, one lens, one run.

  python tools/render_depth_grad_bench.py [--out profiles/render_depth_grad/bench.json] [--reps 10] [--warm 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from conftest import make_lens  # noqa: E402
from render_layers_bench import DEV, DP, WVLN, kernel_times, ramp_depth, texture  # noqa: E402

from sdirt_amd.render_rt import layer_batch, layer_depth_grad_batch, layers_from_rgbd, uniform_layer_depths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_depth_grad", "bench.json"))
    ap.add_argument("--reps", type=int, default=10, help="timed rounds")
    ap.add_argument("--warm", type=int, default=5, help="untimed calls of every kernel before the first round")
    a = ap.parse_args()
    lens = make_lens("rf50mm", DEV)
    torch.manual_seed(0)
    lens.refocus(-1000 + lens.d_sensor)
    lens.prepare_sensor(sensor_res=(512, 768), sensor_size=(24.0, 36.0))
    H, W = lens.sensor_res
    img = texture(H, W)[0].contiguous()                        # [3, H, W], shared by all layers
    res = {"sensor": [H, W], "dp": DP, "wvln": WVLN, "spp": 64, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    torch.manual_seed(1)
    pz, pr = lens.exit_pupil()
    o2 = lens.sample_pupil((H, W), 64, pupilr=pr, pupilz=pz)
    x2, y2 = o2[..., 0].contiguous(), o2[..., 1].contiguous()
    del o2
    gnum = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(DEV)
    depth = ramp_depth(H, W)
    mid = -1500.0
    scenes = {"L1_opaque": ([mid], torch.ones(1, H, W, device=DEV))}
    for L in (4, 8):
        zs = uniform_layer_depths(depth, L)
        scenes[f"L{L}_rgbd"] = (zs, layers_from_rgbd(depth, zs))
    calls, live, grads = [], {}, {}
    for key, (zs, alpha) in scenes.items():
        inv = [1.0 / (float(lens.calc_scale_ray(z)) * lens.pixel_size) for z in zs]          # Wt == W
        fwd = layer_batch(lens, alpha, img, zs, inv, x2, y2, DP, WVLN, landing=True)
        live[key] = (int((fwd["landing"][0] != 0).sum()), int(fwd["landing"][0].numel()))
        trips = fwd["trips"]
        del fwd
        common = (zs, inv, x2, y2)
        grads[key] = layer_depth_grad_batch(lens, alpha, img, *common, trips, gnum, DP, WVLN)[:, 0].tolist()
        calls.append((f"{key}_forward", "render_layers",
                      lambda alpha=alpha, c=common: layer_batch(lens, alpha, img, *c, DP, WVLN, check_alpha=False)))
        calls.append((f"{key}_backward_depth", "render_layers_depth_grad",
                      lambda alpha=alpha, c=common, t=trips: layer_depth_grad_batch(lens, alpha, img, *c, t, gnum, DP, WVLN)))
        if key == "L1_opaque":
            calls.append((f"{key}_backward_depth_null_alpha", "render_layers_depth_grad",
                          lambda c=common, t=trips: layer_depth_grad_batch(lens, None, img, *c, t, gnum, DP, WVLN)))
    res.update(kernel_times(lens, calls, a.warm, a.reps))
    res["timing"] = {"warm_calls_each": a.warm, "rounds": a.reps, "order_in_a_round": [c[0] for c in calls]}
    for key in scenes:
        fwd = res[f"{key}_forward"]
        fwd["layer_depths"] = scenes[key][0]
        for suffix in ("backward_depth", "backward_depth_null_alpha"):
            row = res.get(f"{key}_{suffix}")
            if row is not None:
                row["ratio_to_forward_at_median"] = row["kernel_ms_median"] / fwd["kernel_ms_median"]
                row["live_rays"], row["rays"] = live[key]
                row["lds_bytes_per_workgroup"] = len(scenes[key][0]) * (2 if "null" in suffix else 4) * 256 * 8 + 1024
        res[f"{key}_backward_depth"]["gdepth"] = grads[key]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
