#!/usr/bin/env python3
"""Times of the recording trace and of the trace's backward kernel beside the plain staged trace, in one process
(DESIGN.md section 7f):

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \\
        python3 tools/trace_grad_bench.py --shape 4096x4096 --steps 5 --warmup 2

One batch of N points x S samples through rf50mm (K = 12): sdirt_trace2sensor (k_trace, the yardstick),
sdirt_trace2sensor_record (k_trace_record), sdirt_trace2sensor_grad (k_trace_grad<.., false>) and
sdirt_trace2sensor_grad_eta (k_trace_grad<.., true>: the eta column as well, DESIGN.md sections 7i and 7l; skipped where
the library has no such entry, so that the script also times a build from before it) with the same trip table and
--precision, every ray given an upstream gradient.  The kernel times are rocprofv3's (*_kernel_stats.csv); the device-event times printed
here include the launches and are a cross-check only.  One JSON line: event times, the bytes each call has to move
(bundle in and out: 28 + 28 per ray; checkpoints: 24 (K + 1) per ray written by the recording trace and read by the
backward, which also reads 4 + 16 per ray), and what that is of 8 TB/s."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdirt_amd import Lensgroup, _lib                        # noqa: E402
from sdirt_amd.basics import Ray, dptr, stream_ptr           # noqa: E402

PEAK = 8e12


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
    ap.add_argument("--shape", default="4096x4096", help="points x samples (also: 64x65536)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="lean", choices=("lean", "ieee"), help="the math policy of every call")
    a = ap.parse_args()
    fl = _lib.PSF_STRICT_IEEE if a.precision == "ieee" else 0
    N, S = (int(v) for v in a.shape.split("x"))
    dev = torch.device("cuda:0")
    lens = Lensgroup(os.path.join(os.path.dirname(_lib.HERE), "sdirt_amd", "data", "rf50mm.json"), sensor_res=(512, 768), device=dev)
    K, M = len(lens.surfaces), N * S
    g = torch.Generator().manual_seed(0)
    pts = torch.cat(((torch.rand(N, 2, generator=g) * 2 - 1) * 0.7, -800.0 - 2200.0 * torch.rand(N, 1, generator=g)), 1)
    src = lens.sample_from_points(lens._points_to_object_now(pts), spp=S)
    h, st = _lib.lib(), stream_ptr(dev)
    handle = lens.dev_lens(src.wvln)
    trips = (C.c_int32 * K)(*lens._fixed_trips_for("max").tolist())
    out = Ray.empty(src.shape, src.wvln, dev, obliq=src.has_obliq)
    ws = torch.empty(h.sdirt_trace2sensor_grad_workspace_bytes(M, K) // 4, dtype=torch.float32, device=dev)
    ray_grad = torch.ones((4, M), dtype=torch.float32, device=dev)
    nwg = h.sdirt_trace2sensor_grad_workgroups(M, torch.cuda.get_device_properties(dev).multi_processor_count)
    partial = torch.empty((nwg, K, 3 + _lib.MAX_AI + 1), dtype=torch.float64, device=dev)       # room for the eta column
    calls = {
        "trace2sensor": lambda: _lib.check(h.sdirt_trace2sensor(handle, trips, fl, float(lens.d_sensor), src.c_rays(), out.c_rays(),
                                                                M, None, st)),
        "record": lambda: _lib.check(h.sdirt_trace2sensor_record(handle, trips, fl, float(lens.d_sensor), src.c_rays(),
                                                                 out.c_rays(), M, None, dptr(ws), st)),
        "grad": lambda: _lib.check(h.sdirt_trace2sensor_grad(handle, trips, fl, float(lens.d_sensor), dptr(ws), out.c_rays().ra,
                                                             dptr(ray_grad), M, dptr(partial), nwg, st)),
    }
    nbytes = {"trace2sensor": 56 * M, "record": (56 + 24 * (K + 1)) * M, "grad": (24 * (K + 1) + 20) * M}
    if hasattr(h, "sdirt_trace2sensor_grad_eta"):
        calls["grad_eta"] = lambda: _lib.check(h.sdirt_trace2sensor_grad_eta(handle, trips, fl, float(lens.d_sensor), dptr(ws),
                                                                             out.c_rays().ra, dptr(ray_grad), M, dptr(partial), nwg, st))
        nbytes["grad_eta"] = nbytes["grad"]
    res = {"shape": [N, S], "precision": a.precision, "surfaces": K, "live": None}
    for name, fn in calls.items():
        t = timed(fn, a.steps, a.warmup)
        res[name] = {"event_s": t, "bytes": nbytes[name], "share_of_8TBps": nbytes[name] / t / PEAK}
    res["live"] = float((out.ra != 0).float().mean())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
