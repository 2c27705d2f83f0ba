#!/usr/bin/env python3
"""SHA-256 of every output buffer of the splat's backward entries, on whichever library SDIRT_AMD_LIB names.

The float64 tests of these entries are tolerance tests: a one-ulp change passes them.  This tool is the evidence that a
change to sdirt_grad.hip left the BITS alone: run it once per library, each in a process of its own, and compare the
HASH lines (--compare does both and writes the two outputs and the verdict).

Inputs: seeded, made on the CPU and copied to the device.  N = 5 points x S = 4101 samples: four slices that do not
divide S, the last workgroup of a point with idle lanes.  The rays are tools/grad_bench.py's (positions spread over the
window, |d.x / d.z| < 0.3, d.y spread like d.x) about non-zero centres, and of every eight consecutive rays one has
ra = 0, one lies outside the window, two have a fractional ra in (0, 1) and four have ra = 1: three quarters are inside
the window with weight.
Cases: r 0.5 and 0.65 x lean and IEEE x ks 21 (grids staged in LDS) and ks 79 (read through L2) x
  sdirt_forward_integral_grad, _focus and _rays, each with both grids, grad_l NULL, grad_r NULL and dp NULL;
  sdirt_dp_energy; sdirt_dp_energy_grad with the partials only, with ray_grad and accumulate = 0, and with
  accumulate = 1 on the buffer _rays filled (both grids).
Every buffer must be finite, and more than half of rows 0 and 1 of every ray_grad that _rays wrote non-zero: a hash of
zeros does not pass.

Usage:  [SDIRT_AMD_LIB=path/to/libsdirt_dp.so] python tools/splat_grad_bits.py
        python tools/splat_grad_bits.py --compare PARENT_LIB TREE_LIB --out profiles/splat_body/bits.txt
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PS, N, S = 0.005, 5, 4101


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def inputs(ks, torch):
    g = torch.Generator().manual_seed(1000 + ks)
    M = S * N
    u = lambda: torch.rand(M, generator=g, dtype=torch.float32) * 2 - 1
    half = (ks / 2 - 1) * PS
    center = (torch.rand((N, 2), generator=g, dtype=torch.float32) * 2 - 1) * 3 * PS
    cls = torch.arange(M) % 8                       # 0: ra = 0; 1: outside the window; 2, 3: fractional ra; 4 - 7: ra = 1
    off_x, off_y = u() * half, u() * half
    off_x = torch.where(cls == 1, torch.full_like(off_x, half + 2 * PS), off_x)
    soa = torch.zeros((7, M), dtype=torch.float32)
    soa[0] = -center[:, 0].repeat_interleave(S) - off_x          # the shifted point -o - c = off
    soa[1] = -center[:, 1].repeat_interleave(S) - off_y
    soa[3], soa[4], soa[5] = u() * 0.3, u() * 0.3, 1.0
    frac = torch.rand(M, generator=g, dtype=torch.float32) * 0.98 + 0.01
    soa[6] = torch.where(cls == 0, torch.zeros(M), torch.where((cls == 2) | (cls == 3), frac, torch.ones(M)))
    gl = torch.randn((N, ks, ks), generator=g, dtype=torch.float32)
    gr = torch.randn((N, ks, ks), generator=g, dtype=torch.float32)
    ge = torch.randn((N, 3), generator=g, dtype=torch.float64)
    return soa, center, gl, gr, ge


def run():
    import torch
    sys.path.insert(0, ROOT)
    from sdirt_amd import _lib
    from sdirt_amd.basics import Ray, dptr, stream_ptr
    dev = torch.device("cuda:0")
    h, st = _lib.lib(), stream_ptr(dev)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    ns = int(h.sdirt_forward_integral_grad_slices(N, S, ncu))
    M = S * N
    print(f"library {os.path.relpath(_lib.LIB_PATH, ROOT)}: N {N} S {S} slices {ns} chunk {-(-S // ns)}")
    assert ns == 4 and S % ns != 0
    bad = []

    def report(name, t, rays_rows=False):
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(t).all())
        note = ""
        ok = finite
        if rays_rows:
            live = float((t[:2] != 0).float().mean())
            note = f"  rows 0-1 non-zero {live:.4f}"
            ok = ok and live > 0.5
        print(f"HASH {name} {sha(t)}  finite {finite}{note}")
        if not ok:
            bad.append(name)

    for ks in (21, 79):
        soa, center, gl, gr, ge = inputs(ks, torch)
        ray = Ray.empty((S, N), device=dev)
        ray.soa[:, :M].copy_(soa)
        center, gl, gr, ge = (t.to(dev) for t in (center, gl, gr, ge))
        for r in (0.5, 0.65):
            for prec, flags in (("lean", 0), ("ieee", _lib.PSF_STRICT_IEEE)):
                dp = _lib.DpParams(0.78, 1.44, 0.3, r)
                tag = f"ks{ks} r{r} {prec}"
                head = (ray.c_rays(), S, N, PS, ks, dptr(center))
                kept = None
                for case, pdp, a, b in (("both", C.byref(dp), gl, gr), ("l_null", C.byref(dp), None, gr),
                                        ("r_null", C.byref(dp), gl, None), ("dp_null", None, gl, gr)):
                    for entry, comps in (("sdirt_forward_integral_grad", 5), ("sdirt_forward_integral_grad_focus", 6)):
                        partial = torch.full((N, ns, comps), float("nan"), dtype=torch.float64, device=dev)
                        _lib.check(getattr(h, entry)(*head, pdp, flags, dptr(a), dptr(b), dptr(partial), ns, st))
                        report(f"{tag} {entry} {case}", partial)
                    partial = torch.full((N, ns, 5), float("nan"), dtype=torch.float64, device=dev)
                    rg = torch.full((4, M), float("nan"), dtype=torch.float32, device=dev)
                    _lib.check(h.sdirt_forward_integral_grad_rays(*head, pdp, flags, dptr(a), dptr(b), dptr(partial), ns,
                                                                  dptr(rg), st))
                    report(f"{tag} sdirt_forward_integral_grad_rays {case} partial", partial)
                    report(f"{tag} sdirt_forward_integral_grad_rays {case} ray_grad", rg, rays_rows=True)
                    if case == "both":
                        kept = rg
                e_head = (ray.c_rays(), S, N, C.byref(dp), flags)
                partial = torch.full((N, ns, 3), float("nan"), dtype=torch.float64, device=dev)
                _lib.check(h.sdirt_dp_energy(*e_head, dptr(partial), ns, st))
                report(f"{tag} sdirt_dp_energy", partial)
                partial = torch.full((N, ns, 3), float("nan"), dtype=torch.float64, device=dev)
                _lib.check(h.sdirt_dp_energy_grad(*e_head, dptr(ge), dptr(partial), ns, None, 0, st))
                report(f"{tag} sdirt_dp_energy_grad partial", partial)
                rg = torch.full((4, M), float("nan"), dtype=torch.float32, device=dev)
                _lib.check(h.sdirt_dp_energy_grad(*e_head, dptr(ge), None, ns, dptr(rg), 0, st))
                report(f"{tag} sdirt_dp_energy_grad ray_grad accumulate=0", rg)
                _lib.check(h.sdirt_dp_energy_grad(*e_head, dptr(ge), None, ns, dptr(kept), 1, st))
                report(f"{tag} sdirt_dp_energy_grad ray_grad accumulate=1", kept, rays_rows=True)
    print(f"buffers that are not finite or mostly zero: {len(bad)} {bad if bad else ''}".rstrip())
    return 1 if bad else 0


def compare(parent, tree, out):
    texts = []
    for lib in (parent, tree):
        env = dict(os.environ, SDIRT_AMD_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            sys.stdout.write(p.stdout + p.stderr)
            return p.returncode or 1
        texts.append(p.stdout)
    hashes = [[l for l in t.splitlines() if l.startswith("HASH ")] for t in texts]
    equal = len(hashes[0]) > 0 and hashes[0] == hashes[1]
    differ = [a for a, b in zip(*hashes) if a != b]
    report = (f"--- parent ({parent})\n{texts[0]}--- tree ({tree})\n{texts[1]}\n"
              f"hashes: {len(hashes[0])} per library, equal between the two libraries: {equal}\n")
    for a in differ:
        report += f"DIFFERS {a[5:a.index('  finite') - 65]}\n"
    sys.stdout.write(report)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(report)
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_LIB", "TREE_LIB"), help="one child process per library")
    ap.add_argument("--out", help="--compare: write both outputs and the verdict here as well")
    args = ap.parse_args()
    sys.exit(compare(*args.compare, args.out) if args.compare else run())


if __name__ == "__main__":
    main()
