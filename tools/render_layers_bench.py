#!/usr/bin/env python3
"""The layered ray-traced render (k_render_layers) measured on one box, one run:

  time    512 x 768 RGB frame behind rf50mm, 64 spp: the kernel's time (HIP events around its launches), median and
          range of --reps launches, for L = 1 (one opaque layer) and for L = 4 and L = 8 of an `extend`ed RGB-D stack
          (layers_from_rgbd of a depth map of smooth ramps and steps), next to render_plane on the same pupil points.
          The four are warmed --warm calls each and then timed in turn, round after round, so that a drift of the
          box cannot pass for a difference between them;
  edge    a two-depth scene -- a foreground bar at -700 mm over a background at -3000 mm, the lens focused at -1000 mm:
          render_rgbd against local_dp_psf_render with per-pixel psf_lr pairs (as tools/render_rt_bench.py builds them,
          each pixel at its own depth), largest and mean absolute difference within KS pixels of the depth edge and away
          from it, at 64 and at 256 spp, and 64 against 256 spp alongside, so that the Monte-Carlo share shows.

Written to profiles/render_layers/bench.json (and printed).  Measurements, no targets: one scene, one lens.

  python tools/render_layers_bench.py [--out profiles/render_layers/bench.json] [--reps 10] [--warm 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import make_lens  # noqa: E402

from sdirt_amd import local_dp_psf_render  # noqa: E402
from sdirt_amd.render_rt import layers_from_rgbd, uniform_layer_depths  # noqa: E402

DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
WVLN = 0.589
KS = 21
NEAR, FAR = -700.0, -3000.0


def texture(H, W):
    """tools/render_rt_bench.py's: smooth noise with a few hard edges, in [0, 1]."""
    g = torch.Generator().manual_seed(0)
    t = torch.nn.functional.interpolate(torch.rand(1, 3, H // 8, W // 8, generator=g), size=(H, W), mode="bilinear")
    t[..., H // 4:H // 4 + 6, :] = 1.0
    t[..., :, W // 3:W // 3 + 6] = 0.0
    return t.clamp(0, 1).to(DEV)


def ramp_depth(H, W):
    """A depth map between NEAR and FAR: a ramp in 1 / depth from left to right with two boxes stepped out of it."""
    inv = torch.linspace(1 / FAR, 1 / NEAR, W)[None, :].repeat(H, 1)
    inv[H // 4:H // 2, W // 8:W // 3] = 1 / NEAR
    inv[H // 2:7 * H // 8, W // 2:3 * W // 4] = 1 / FAR
    return (1.0 / inv).to(DEV)


def kernel_times(lens, calls, warm, reps):
    """calls: [(key, name of the kernel's event bracket, function)].  Every call runs `warm` times untimed (the trip table
    is learnt, the lens uploaded, the clocks up), then `reps` rounds are timed, each round running the calls one after
    the other in the listed order: a drift of the box falls on all of them alike and not on the one measured first.
    -> key -> the kernel time of every round (HIP events around the launches of the call, summed), median and range."""
    for _ in range(warm):
        for _, _, call in calls:
            call()
    ms = {key: [] for key, _, _ in calls}
    for _ in range(reps):
        for key, name, call in calls:
            lens.kernel_events = {}
            call()
            torch.cuda.synchronize()
            ms[key].append((sum(e0.elapsed_time(e1) for e0, e1 in lens.kernel_events[name]), len(lens.kernel_events[name])))
    lens.kernel_events = None
    out = {}
    for key, rows in ms.items():
        ev = [t for t, _ in rows]
        out[key] = {"kernel_ms_median": float(np.median(ev)), "kernel_ms_min": float(min(ev)), "kernel_ms_max": float(max(ev)),
                    "kernel_ms_all": [round(v, 3) for v in ev], "launches_per_call": rows[0][1]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_layers", "bench.json"))
    ap.add_argument("--reps", type=int, default=10, help="timed rounds")
    ap.add_argument("--warm", type=int, default=10, help="untimed calls of every kernel before the first round")
    a = ap.parse_args()
    lens = make_lens("rf50mm", DEV)
    torch.manual_seed(0)
    lens.refocus(-1000 + lens.d_sensor)
    lens.prepare_sensor(sensor_res=(512, 768), sensor_size=(24.0, 36.0))
    H, W = lens.sensor_res
    img = texture(H, W)
    res = {"sensor": [H, W], "dp": DP, "wvln": WVLN, "ks": KS, "spp": 64, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}

    torch.manual_seed(1)
    pz, pr = lens.exit_pupil()
    o2 = torch.cat([lens.sample_pupil((H, W), 64, pupilr=pr, pupilz=pz) for _ in range(4)])
    x2, y2 = o2[..., 0].contiguous(), o2[..., 1].contiguous()
    del o2
    pts64 = (x2[:64], y2[:64])

    # ---- time: the plane kernel, one opaque layer, 4 and 8 layers of an extended RGB-D stack
    torch.manual_seed(3)
    scale_of = {}

    def scale(z):
        if z not in scale_of:
            scale_of[z] = float(lens.calc_scale_ray(z))
        return scale_of[z]

    mid = -1500.0
    calls = [("render_plane", "render_plane", lambda: lens.render_plane(
                 img, mid, spp=64, dp=DP, wvln=WVLN, scale=scale(mid), pupil_points=pts64)),
             ("render_layers_L1_opaque", "render_layers", lambda: lens.render_layers(
                 img[0], torch.ones(1, H, W, device=DEV), [mid], spp=64, dp=DP, wvln=WVLN, scales=[scale(mid)],
                 pupil_points=pts64))]
    depth = ramp_depth(H, W)
    stacks = {}
    for L in (4, 8):
        zs = uniform_layer_depths(depth, L)
        stacks[L] = (zs, layers_from_rgbd(depth, zs), [scale(z) for z in zs])
        calls.append((f"render_layers_L{L}_rgbd", "render_layers", lambda L=L: lens.render_layers(
            img[0], stacks[L][1], stacks[L][0], spp=64, dp=DP, wvln=WVLN, scales=stacks[L][2], pupil_points=pts64)))
    res.update(kernel_times(lens, calls, a.warm, a.reps))
    res["timing"] = {"warm_calls_each": a.warm, "rounds": a.reps, "order_in_a_round": [c[0] for c in calls]}
    for L in (4, 8):
        res[f"render_layers_L{L}_rgbd"]["layer_depths"] = stacks[L][0]
        res[f"render_layers_L{L}_rgbd"]["own_layer_share"] = [
            float(v) for v in layers_from_rgbd(depth, stacks[L][0], extend=False).mean((1, 2))]

    # ---- edge: a bar at NEAR over a background at FAR, ray traced with occlusion against the per-pixel PSF render
    depth = torch.full((1, 1, H, W), FAR, device=DEV)
    bar = slice(W // 2 - W // 16, W // 2 + W // 16)
    depth[..., bar] = NEAR
    zs = [NEAR, FAR]
    scales = [scale(z) for z in zs]

    def traced(spp):
        return lens.render_rgbd(img, depth, layer_depths=zs, spp=spp, dp=DP, wvln=WVLN, scales=scales,
                                pupil_points=(x2[:spp], y2[:spp]))

    L64, R64 = traced(64)
    L256, R256 = traced(256)
    gx, gy = torch.meshgrid(torch.linspace(-1, 1, W), torch.linspace(1, -1, H), indexing="xy")
    pts = torch.stack((gx.to(DEV), gy.to(DEV), depth[0, 0]), -1).reshape(-1, 3)
    psf = torch.empty((H * W, 2, KS, KS), dtype=torch.float32, device=DEV)
    torch.manual_seed(2)
    step = 16384
    for n0 in range(0, H * W, step):
        lens.psf_lr(pts[n0:n0 + step], ks=KS, wvln=WVLN, dp=DP, normalize=False, out=psf[n0:n0 + step])
    psf /= psf.sum((-1, -2), keepdim=True).clamp_min(1e-30)
    lr = local_dp_psf_render(img, psf.view(1, H, W, 2, KS, KS), kernel_size=KS)
    PL, PR = lr[:, :3], lr[:, 3:]
    del psf
    cols = torch.arange(W, device=DEV)
    near_edge = ((cols - bar.start).abs() <= KS) | ((cols - bar.stop).abs() <= KS)
    inner = torch.zeros(W, dtype=torch.bool, device=DEV)
    inner[KS:-KS] = True                                      # away from the frame, where the convolution pads
    at_edge, away = near_edge & inner, ~near_edge & inner

    def diff(A, B, C, D):
        d = torch.stack((A - C, B - D)).abs()[..., KS:-KS, :]
        return {"max_abs_at_edge": float(d[..., at_edge].max()), "mean_abs_at_edge": float(d[..., at_edge].mean()),
                "max_abs_away": float(d[..., away].max()), "mean_abs_away": float(d[..., away].mean())}

    res["edge_scene"] = {
        "near": NEAR, "far": FAR, "bar_columns": [bar.start, bar.stop], "edge_band_px": KS, "scales": scales,
        "raytraced_64spp_vs_psf": diff(L64, R64, PL, PR), "raytraced_256spp_vs_psf": diff(L256, R256, PL, PR),
        "raytraced_64_vs_256spp": diff(L64, R64, L256, R256),
        "left_right_mean_abs_at_edge": {"raytraced_256spp": float((L256 - R256).abs()[..., KS:-KS, :][..., at_edge].mean()),
                                        "psf": float((PL - PR).abs()[..., KS:-KS, :][..., at_edge].mean())}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
