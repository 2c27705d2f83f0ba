#!/usr/bin/env python3
"""The layered render's backward (k_render_layers_grad) measured on one box, one run:

  512 x 768 RGB frame behind rf50mm, 64 spp, the three planes sharing one trace, default dp, on the scenes of
  tools/render_layers_bench.py: one opaque layer, and the `extend`ed RGB-D stacks of 4 and 8 layers.  Per scene the
  forward kernel (k_render_layers) and the backward kernel with both gradients, with the colour gradient only and
  -- one opaque layer -- with a null alpha (render_plane's backward), HIP events around the launches.  All calls are
  warmed --warm times each and then timed in turn, round after round (a drift of the box falls on all alike); median
  and range of --reps rounds.

  Next to each backward time: the float64 adds it issued (counted from the forward's landing record by the torch
  restatement's lookup: 4 per colour plane and layer with g_l != 0, 4 per layer with T_l != 0), and issued adds x 8 B /
  time -- to be read next to the ~1.3 TB/s the hardware guide gives for fp32 atomic adds of 256 contiguous bytes; for
  scattered 8-byte float64 adds nobody had a figure.  The kernel also traces every ray again, so the rate is a lower
  bound on what the atomics alone sustain.

Written to profiles/render_layers_grad/bench.json (and printed).  Measurements, no targets.

  python tools/render_layers_grad_bench.py [--out profiles/render_layers_grad/bench.json] [--reps 10] [--warm 5]
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

from sdirt_amd.render_rt import (_read_taps, _taps_float64, layer_batch, layer_grad_batch, layers_from_rgbd,  # noqa: E402
                                 uniform_layer_depths)


def issued_adds(land, alpha, inv, planes, step=4):
    """(colour adds, coverage adds) of one backward launch, from the forward's landing record, `step` samples at a time."""
    L = alpha.shape[0]
    Ht, Wt = alpha.shape[-2:]
    colour = coverage = 0
    for s0 in range(0, land.shape[1], step):
        part = land[:, s0:s0 + step]
        live = part[0] != 0
        T = torch.ones(part[0].shape, dtype=torch.float64, device=land.device)
        for l in range(L):
            idx, w = _taps_float64(part[3 + 2 * l], part[4 + 2 * l], inv[l], live, Ht, Wt)
            a = _read_taps(alpha[l:l + 1], idx, w, live)[0]
            colour += 4 * planes * int((live & (T * a != 0)).sum())
            coverage += 4 * int((live & (T != 0)).sum())
            T = T * (1 - a)
    return colour, coverage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_layers_grad", "bench.json"))
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
    torch.manual_seed(3)
    gnum = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(DEV)
    depth = ramp_depth(H, W)
    mid = -1500.0
    scenes = {"L1_opaque": ([mid], torch.ones(1, H, W, device=DEV))}
    for L in (4, 8):
        zs = uniform_layer_depths(depth, L)
        scenes[f"L{L}_rgbd"] = (zs, layers_from_rgbd(depth, zs))
    calls, adds = [], {}
    for key, (zs, alpha) in scenes.items():
        inv = [1.0 / (float(lens.calc_scale_ray(z)) * lens.pixel_size) for z in zs]          # Wt == W
        fwd = layer_batch(lens, alpha, img, zs, inv, x2, y2, DP, WVLN, landing=True)
        adds[key] = issued_adds(fwd["landing"], alpha, inv, 3)
        trips = fwd["trips"]
        del fwd
        ga = torch.zeros(alpha.shape, dtype=torch.float64, device=DEV)
        gt = torch.zeros(img.shape, dtype=torch.float64, device=DEV)
        common = (zs, inv, x2, y2)
        calls.append((f"{key}_forward", "render_layers",
                      lambda alpha=alpha, c=common: layer_batch(lens, alpha, img, *c, DP, WVLN, check_alpha=False)))
        calls.append((f"{key}_backward_both", "render_layers_grad",
                      lambda alpha=alpha, c=common, t=trips, ga=ga, gt=gt: layer_grad_batch(
                          lens, alpha, img, *c, t, gnum, DP, WVLN, galpha=ga, gtex=gt)))
        calls.append((f"{key}_backward_colour", "render_layers_grad",
                      lambda alpha=alpha, c=common, t=trips, gt=gt: layer_grad_batch(
                          lens, alpha, img, *c, t, gnum, DP, WVLN, galpha=False, gtex=gt)))
        if key == "L1_opaque":
            calls.append((f"{key}_backward_null_alpha", "render_layers_grad",
                          lambda c=common, t=trips, gt=gt: layer_grad_batch(lens, None, img, *c, t, gnum, DP, WVLN, gtex=gt)))
    res.update(kernel_times(lens, calls, a.warm, a.reps))
    res["timing"] = {"warm_calls_each": a.warm, "rounds": a.reps, "order_in_a_round": [c[0] for c in calls]}
    for key, (colour, coverage) in adds.items():
        for suffix, n in (("backward_both", colour + coverage), ("backward_colour", colour), ("backward_null_alpha", colour)):
            row = res.get(f"{key}_{suffix}")
            if row is not None:
                row["atomic_adds_issued"] = n
                row["atomic_bytes_per_s_at_median"] = n * 8 / (row["kernel_ms_median"] * 1e-3)
        res[f"{key}_forward"]["layer_depths"] = scenes[key][0]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
