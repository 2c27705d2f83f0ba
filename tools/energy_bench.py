#!/usr/bin/env python3
"""Time the energy kernels (sdirt_dp_energy, sdirt_dp_energy_grad) on their own, beside the staged splat on the same
rays, and psf_lr(energy=True) against the same staged call without it.

Kernels: 4096 points x 4096 samples of synthetic sensor-plane rays (|x_tan| < 0.3, every ray valid, positions spread
over a ks 65 window), the reference's default stack with r = 0.5 unless --big.  Device events around `iters`
back-to-back calls (launches included).  Counted bytes: the three ray arrays the energy kernels read (d.x, d.z, ra:
12 B per ray), the two rows the ray-gradient forms write (8 B per ray; accumulate = 1 reads them as well, accumulate = 0
writes all four) and the float64 partials.  --only NAME[,NAME...] runs those entries alone, each in a loop of its own,
for a kernel trace (each has a kernel name of its own).

psf_lr: rf50mm, `--points` field points at `--spp` samples, ks 150 (above SDIRT_MAX_KS, so that the call without the
energy is the staged chain as well), fixed pupil samples, the two calls alternating in one process.

Usage:  python tools/energy_bench.py [--iters 50] [--big] [--ieee] [--only energy,grad_partial,grad_rays,grad_rays_acc]
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
DEV = torch.device("cuda:0")


def timed(launch, iters):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernels(N, S, iters, r, flags, only=None):
    g = torch.Generator(device=DEV).manual_seed(0)
    ks, M = 65, S * N
    ray = Ray.empty((S, N), device=DEV)
    half = (ks / 2 - 1) * PS
    ray.soa[0, :M] = (torch.rand(M, device=DEV, generator=g) * 2 - 1) * half
    ray.soa[1, :M] = (torch.rand(M, device=DEV, generator=g) * 2 - 1) * half
    ray.soa[2, :M] = 0.0
    ray.soa[3, :M] = (torch.rand(M, device=DEV, generator=g) * 2 - 1) * 0.3
    ray.soa[4, :M] = 0.0
    ray.soa[5, :M] = 1.0
    ray.soa[6, :M] = 1.0
    h, st = _lib.lib(), stream_ptr(DEV)
    ncu = torch.cuda.get_device_properties(DEV).multi_processor_count
    ns = int(h.sdirt_forward_integral_grad_slices(N, S, ncu))
    dp = _lib.DpParams(0.78, 1.44, 0.3, r)
    partial = torch.empty((N, ns, 3), dtype=torch.float64, device=DEV)
    ge = torch.randn((N, 3), dtype=torch.float64, device=DEV, generator=g)
    rg = torch.zeros((4, M), dtype=torch.float32, device=DEV)
    center = torch.zeros((N, 2), dtype=torch.float32, device=DEV)
    lg, rgrid = (torch.empty((N, ks, ks), dtype=torch.float32, device=DEV) for _ in range(2))
    part_bytes = 24 * N * ns
    entries = {
        "energy": (lambda: _lib.check(h.sdirt_dp_energy(ray.c_rays(), S, N, C.byref(dp), flags, dptr(partial), ns, st)),
                   12 * M + part_bytes),
        "grad_partial": (lambda: _lib.check(h.sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dp), flags, dptr(ge),
                                                                   dptr(partial), ns, None, 0, st)), 12 * M + part_bytes),
        "grad_rays": (lambda: _lib.check(h.sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dp), flags, dptr(ge), None, ns,
                                                                dptr(rg), 0, st)), 28 * M),
        "grad_rays_acc": (lambda: _lib.check(h.sdirt_dp_energy_grad(ray.c_rays(), S, N, C.byref(dp), flags, dptr(ge), None, ns,
                                                                    dptr(rg), 1, st)), 28 * M),
        "forward_integral": (lambda: _lib.check(h.sdirt_forward_integral(ray.c_rays(), S, N, PS, ks, dptr(center), C.byref(dp),
                                                                         flags, dptr(lg), dptr(rgrid), st)),
                             20 * M + 8 * ks * ks * N),
    }
    out = []
    for name, (launch, nbytes) in entries.items():
        if only is not None and name not in only.split(","):
            continue
        ms = timed(launch, iters)
        if name == "energy":
            first = partial.clone()
            launch()
            torch.cuda.synchronize()
            assert torch.equal(first, partial), "the energy kernel is not run-to-run identical"
        out.append(dict(entry=name, points=N, spp=S, slices=ns, ms=round(ms, 4), gbytes=round(nbytes / 1e9, 4),
                        gb_per_s=round(nbytes / ms / 1e6, 1), frac_of_8tbs=round(nbytes / ms / 1e6 / 8000, 3)))
    return out


def psf_calls(points, spp, iters):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path.insert(0, os.path.join(root, "tests"))
    from conftest import load_state, make_lens
    lens = make_lens("rf50mm", "cuda:0", load_state("rf50mm"))
    g = torch.Generator().manual_seed(1)
    pts = torch.cat(((torch.rand(points, 2, generator=g) * 2 - 1) * 0.9, -300.0 - 3000.0 * torch.rand(points, 1, generator=g)), 1)
    torch.manual_seed(2)
    with torch.no_grad():
        lens.psf_lr(pts[:2], ks=21, spp=spp)
    x2, y2, xc, yc = (t.clone() for t in lens.last_pupil_points)
    kw = dict(ks=_lib.MAX_KS + 9, dp=(0.78, 1.44, 0.3, 0.5), pupil_xy=(x2, y2), center_pupil_xy=(xc, yc))
    plain = lambda: lens.psf_lr(pts, **kw)
    with_e = lambda: lens.psf_lr(pts, energy=True, **kw)
    rounds = []
    with torch.no_grad():
        for _ in range(3):                         # alternating, in one process
            rounds.append((round(timed(plain, iters), 4), round(timed(with_e, iters), 4)))
    return dict(entry="psf_lr", points=points, spp=x2.numel(), ks=kw["ks"], ms_plain=[a for a, _ in rounds],
                ms_energy=[b for _, b in rounds])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--big", action="store_true", help="r = 0.65 (big-r model)")
    ap.add_argument("--ieee", action="store_true", help="SDIRT_PSF_STRICT_IEEE")
    ap.add_argument("--only", default=None, help="these kernel entries only, comma-separated (for a kernel trace)")
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--spp", type=int, default=4096)
    args = ap.parse_args()
    r = 0.65 if args.big else 0.5
    flags = _lib.PSF_STRICT_IEEE if args.ieee else 0
    for res in kernels(4096, 4096, args.iters, r, flags, args.only):
        res.update(r=r, precision="ieee" if args.ieee else "lean")
        print(json.dumps(res), flush=True)
    if args.only is None:
        print(json.dumps(psf_calls(args.points, args.spp, max(args.iters // 5, 5))), flush=True)


if __name__ == "__main__":
    main()
