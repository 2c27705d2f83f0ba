#!/usr/bin/env python3
"""The reference's autograd gradients of its dual-pixel PSFs (f27_dp_grad): the yardstick of the gradient path.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (see oracle/_refimport.py); it imports the reference
through oracle/gen_golden.py (lens construction with the frozen pupil) and produces numbers only.  The file is not
committed: tests/golden/ holds exactly what the generators under oracle/ write (tests/test_oracle_golden.py::
test_the_fixtures_regenerate_byte_for_byte).  tests/test_dp_grad_cpu.py computes the cases afresh (cases()), and the
file this script writes can be dropped into tests/golden/ by hand for a GPU comparison run.  For every case, one psf_diff call of the reference (deeplens/optics.py:934-996) on rf50mm with
param_list = [h, f, w, r, direct], h / f / w 0-d tensors that require grad, and the loss sum(G * psf) for a fixed
upstream weight G; .backward() gives dL/dh, dL/df, dL/dw and, with center=False, dL/dpoints (through the pinhole
centres, optics.py:973-976).  Each case runs twice on the same pupil samples: as the reference runs (fp32 rays,
fp32 parameters) and with the rays that reach forward_integral, the centres and h, f, w cast to float64 (and
float64 as torch's default dtype inside forward_integral, so that its grids and r are float64 too).  The
difference of the two is the reference's own spread.  Stored per case (prefix c<i>_):
  points, pupil_x2 / pupil_y2 (primary) and pupil_xc / pupil_yc (chief ray, center=True) for the pupil hand-off,
  dp = [h, f, w, r], direct (0 = 'l', 1 = 'r'), center, G, psf (fp32 run), grad32 / grad64 = [dh, df, dw],
  gpts32 = dL/dpoints[:, :2] and gcen64 = float64 dL/dpointc_ref [N, 2] (center=False), and the sensor-plane rays of
  the fp32 run (ox, oy, dx, dz, ra [spp, N]) with the centres pointc [N, 2] they were splatted around.

Usage:  python tools/gen_golden_dp_grad.py --out DIR
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import gen_golden as gg  # noqa: E402  (imports the reference through _refimport)

ref_optics = gg.ref_optics

KS, SPP, SEED = 21, 1024, 27
POINTS = np.array([[0.0, 0.0, -1500.0], [0.35, -0.2, -1200.0], [-0.6, 0.45, -2500.0]], np.float32)
# (r, direct, center): both area models, both directions, both centre rules
CASES = [(0.5, "l", True), (0.65, "r", True), (0.5, "r", False), (0.65, "l", False)]
DP = (0.78, 1.44, 0.3)


class Splat64:
    """Wraps the reference's forward_integral (looked up in optics' globals): records the rays and centres it gets
    and, with cast=True, hands them over as float64 (the centres through a differentiable cast, with a hook that
    keeps their float64 gradient)."""

    def __init__(self, cast):
        self.cast, self.rays, self.center, self.gcen = cast, None, None, None

    def __enter__(self):
        self._fi = ref_optics.forward_integral
        rec = self

        def fi(ray, ps, ks, pointc_ref=None, interpolate=False, param_list=None):
            rec.rays = [t.detach().numpy().copy() for t in (ray.o[..., 0], ray.o[..., 1], ray.d[..., 0],
                                                              ray.d[..., 2], ray.ra)]
            rec.center = pointc_ref.detach().numpy().copy()
            if rec.cast:
                ray.o, ray.d, ray.ra = ray.o.double(), ray.d.double(), ray.ra.double()
                pointc_ref = pointc_ref.double()
                if pointc_ref.requires_grad:
                    pointc_ref.register_hook(lambda g: setattr(rec, "gcen", g.detach().numpy().copy()))
                # the grids the splat allocates (torch.zeros(ks, ks), monte_carlo.py:224) and r (torch.tensor(r),
                # :167) in float64 as well
                torch.set_default_dtype(torch.float64)
            try:
                return rec._fi(ray, ps, ks, pointc_ref=pointc_ref, interpolate=interpolate, param_list=param_list)
            finally:
                torch.set_default_dtype(torch.float32)
        ref_optics.forward_integral = fi
        return self

    def __exit__(self, *exc):
        ref_optics.forward_integral = self._fi


class Draws:
    """Records the uniform draws (torch.rand) and the pupil sample points (the (x2, y2, z2) stack of
    optics.py:488) of one call -- or, given the draws of an earlier call, replays them."""

    def __init__(self, replay=None):
        self.replay, self.rand, self.pupil = (iter(replay) if replay is not None else None), [], []

    def __enter__(self):
        self._rand, self._stack = torch.rand, torch.stack
        rec = self

        def rand(*a, **k):
            out = torch.from_numpy(next(rec.replay).copy()) if rec.replay is not None else rec._rand(*a, **k)
            rec.rand.append(out.numpy().copy())
            return out

        def stack(tensors, *a, **k):
            if len(a) == 1 and a[0] == 1 and len(tensors) == 3 and all(t.dim() == 1 for t in tensors):
                rec.pupil.append((tensors[0].detach().numpy().copy(), tensors[1].detach().numpy().copy()))
            return rec._stack(tensors, *a, **k)
        torch.rand, torch.stack = rand, stack
        return self

    def __exit__(self, *exc):
        torch.rand, torch.stack = self._rand, self._stack


def run(lens, r, direct, center, G, pupil, dtype):
    """One psf_diff + backward.  pupil=None: draw (and record) the samples; else replay them."""
    pts = torch.tensor(POINTS, requires_grad=not center)
    h, f, w = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in DP)
    gg.set_seed(SEED)
    with Draws(pupil) as rec, Splat64(cast=dtype == torch.float64) as sp:
        psf = lens.psf_diff(points=pts, ks=KS, spp=SPP, center=center, param_list=[h, f, w, r, direct])
    loss = (torch.from_numpy(G).to(psf.dtype) * psf).sum()
    loss.backward()
    out = dict(psf=psf.detach().float().numpy(), grad=np.array([float(h.grad), float(f.grad), float(w.grad)]),
               rand=rec.rand, pupil=rec.pupil, rays=sp.rays, center=sp.center, gcen=sp.gcen)
    if not center:
        out["gpts"] = pts.grad[:, :2].numpy().copy()
    return out


def cases(which=None, check_repeat=True):
    """-> {key: array} of the cases (all, or the indices in `which`), keys prefixed c<i>_."""
    lens = gg.build_lens("rf50mm")
    rng = np.random.default_rng(SEED)
    d = dict(n_cases=np.int32(len(CASES)), ks=np.int32(KS), spp=np.int32(SPP))
    for i, (r, direct, center) in enumerate(CASES):
        G = rng.standard_normal((len(POINTS), KS, KS)).astype(np.float32)
        if which is not None and i not in which:
            continue
        a = run(lens, r, direct, center, G, None, torch.float32)
        if check_repeat:
            a2 = run(lens, r, direct, center, G, a["rand"], torch.float32)
            assert np.array_equal(a["psf"], a2["psf"]) and np.array_equal(a["grad"], a2["grad"]), "not reproducible"
        b = run(lens, r, direct, center, G, a["rand"], torch.float64)
        p = f"c{i}_"
        d[p + "points"] = POINTS
        d[p + "dp"] = np.array([*DP, r])
        d[p + "direct"] = np.int32(direct != "l")
        d[p + "center"] = np.int32(center)
        d[p + "G"] = G
        d[p + "psf"] = a["psf"]
        d[p + "grad32"], d[p + "grad64"] = a["grad"], b["grad"]
        d[p + "pupil_x2"], d[p + "pupil_y2"] = a["pupil"][0]
        if center:
            d[p + "pupil_xc"], d[p + "pupil_yc"] = a["pupil"][1]
        else:
            d[p + "gpts32"], d[p + "gcen64"] = a["gpts"], b["gcen"]
        for k, v in zip(("ox", "oy", "dx", "dz", "ra"), a["rays"]):
            d[p + k] = v
        d[p + "pointc"] = a["center"]
        spread = np.abs(a["grad"] - b["grad"]) / np.abs(b["grad"])
        print(f"case {i} r={r} direct={direct} center={center}: grad32={a['grad']} grad64={b['grad']} "
              f"spread={spread}")
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    d = cases()
    path = os.path.join(args.out, "f27_dp_grad.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
