#!/usr/bin/env python3
"""Times of the object-point walk, in one process:

    python3 tools/point_grad_bench.py --shape 256x4096 --steps 50 --warmup 5

One batch of N points x S samples through rf50mm (K = 12), recorded once.
 1. sdirt_trace2sensor_grad_points (k_trace_grad_points) against sdirt_trace2sensor_grad (k_trace_grad: unchanged by this
    feature, the yardstick) on the same record, every live ray given an upstream gradient: device events around
    `steps` back-to-back calls.
 2. The whole psf_lr(point_grad=True) forward and backward (chief-ray centres, ks 21) against the same call with only
    h requiring a gradient: device events around `steps` calls each.
One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdirt_amd import Lensgroup, _lib                        # noqa: E402
from sdirt_amd.basics import Ray, dptr, stream_ptr           # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="256x4096", help="points x samples")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", type=int, default=21)
    ap.add_argument("--precision", default="lean", choices=("lean", "ieee"), help="the math policy of the three entries")
    a = ap.parse_args()
    fl = _lib.PSF_STRICT_IEEE if a.precision == "ieee" else 0
    N, S = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    lens = Lensgroup(os.path.join(os.path.dirname(_lib.HERE), "sdirt_amd", "data", "rf50mm.json"), sensor_res=(512, 768), device=dev)
    K, M = len(lens.surfaces), N * S
    g = torch.Generator().manual_seed(0)
    pts = torch.cat(((torch.rand(N, 2, generator=g) * 2 - 1) * 0.7, -800.0 - 2200.0 * torch.rand(N, 1, generator=g)), 1)
    pupil_z, pupil_r = lens.entrance_pupil()
    x2, y2 = lens._pupil_samples(S, pupil_r)
    po = lens._points_to_object_now(pts)
    src = Ray.empty((S, N), 0.589, dev)
    h, st = _lib.lib(), stream_ptr(dev)
    _lib.check(h.sdirt_sample_rays(dptr(po), N, dptr(x2), dptr(y2), S, float(pupil_z), src.c_rays(), st))
    handle = lens.dev_lens(src.wvln)
    trips = (C.c_int32 * K)(*lens._fixed_trips_for("max").tolist())
    out = Ray.empty(src.shape, src.wvln, dev, obliq=src.has_obliq)
    ws = torch.empty(h.sdirt_trace2sensor_grad_workspace_bytes(M, K) // 4, dtype=torch.float32, device=dev)
    _lib.check(h.sdirt_trace2sensor_record(handle, trips, fl, float(lens.d_sensor), src.c_rays(), out.c_rays(), M, None, dptr(ws), st))
    ray_grad = torch.ones((4, M), dtype=torch.float32, device=dev)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    nwg = h.sdirt_trace2sensor_grad_workgroups(M, ncu)
    ns = h.sdirt_forward_integral_grad_slices(N, S, ncu)
    partial = torch.empty((nwg, K, 3 + _lib.MAX_AI), dtype=torch.float64, device=dev)
    p_partial = torch.empty((N, ns, 3), dtype=torch.float64, device=dev)
    calls = {
        "grad": lambda: _lib.check(h.sdirt_trace2sensor_grad(handle, trips, fl, float(lens.d_sensor), dptr(ws), out.c_rays().ra,
                                                             dptr(ray_grad), M, dptr(partial), nwg, st)),
        "grad_points": lambda: _lib.check(h.sdirt_trace2sensor_grad_points(
            handle, trips, fl, float(lens.d_sensor), dptr(ws), out.c_rays().ra, dptr(ray_grad), S, N, dptr(x2), dptr(y2),
            float(pupil_z), dptr(p_partial), ns, st)),
    }
    res = {"shape": [N, S], "precision": a.precision, "surfaces": K, "workgroups": {"grad": int(nwg), "grad_points": int(N * ns)},
           "live": float((out.ra != 0).float().mean())}
    for name, fn in calls.items():
        res[name + "_event_s"] = timed(fn, a.steps, a.warmup)
    res["points_over_params"] = res["grad_points_event_s"] / res["grad_event_s"]
    # the whole call
    DP = (0.78, 1.44, 0.3, 0.5)
    xc, yc = lens._pupil_samples(2048, lens.entrance_pupil(shrink_pupil=True)[1])
    G = torch.randn((N, a.ks, a.ks), generator=g).to(dev)
    kw = dict(ks=a.ks, pupil_xy=(x2, y2), center_pupil_xy=(xc, yc))

    def with_points():
        p = pts.clone().requires_grad_()
        L, R = lens.psf_lr(p, dp=DP, point_grad=True, **kw)
        ((G * L).sum() + (G * R).sum()).backward()

    def with_h():
        hh = torch.tensor(DP[0], requires_grad=True)
        L, R = lens.psf_lr(pts, dp=(hh, *DP[1:]), **kw)
        ((G * L).sum() + (G * R).sum()).backward()
    res["call_point_grad_s"] = timed(with_points, a.steps, a.warmup)
    res["call_h_grad_s"] = timed(with_h, a.steps, a.warmup)
    res["call_ratio"] = res["call_point_grad_s"] / res["call_h_grad_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
