#!/usr/bin/env python3
"""The reference's own float64 autograd gradient of a dual-pixel PSF in the sensor position: the yardstick of the
float64 restatement tests/focus_f64.py.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (see oracle/_refimport.py); it imports the reference
through oracle/gen_golden.py (lens construction with the frozen pupil) and produces numbers only; nothing it makes is
committed.  tests/test_focus_grad_cpu.py computes the cases afresh (run()).

The reference has no sensor-position parameter.  Here lens.d_sensor is a 0-d float64 tensor that requires a gradient,
and one psf_diff call runs with
  * its trace in fp32 as it ships (no gradient: the rays are sampled under no_grad), the traced bundle then cast to
    float64 BEFORE Ray.propagate_to(lens.d_sensor), so that the propagation, forward_integral (float64 as torch's
    default dtype inside it, tools/gen_golden_dp_grad.Splat64) and the max-normalisation are the reference's own
    operations in float64;
  * psf_center either as it ships (under no_grad: the centre is a constant) or, `centre_in_graph`, replaced by the
    same computation without no_grad -- chief rays sampled under no_grad, trace2sensor, the ra-weighted mean.
Recorded: the sensor-plane bundles (primary, chief) that forward_integral and the centre were computed from, as
float64 arrays (o.x, o.y, d.x, d.y, d.z, ra) [spp, N], the centres, the PSF, the loss and d loss / d d_sensor.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_dp_grad as dg  # noqa: E402  (imports the reference through oracle/gen_golden.py)

gg, ref_optics = dg.gg, dg.ref_optics

KS, SPP, SEED = dg.KS, dg.SPP, 41
POINTS, CASES, DP = dg.POINTS, dg.CASES, dg.DP
# the issue's probe: four points whose PSFs lie wholly inside a 21-pixel window (depth + d_sensor is added by the caller)
PROBE_POINTS = np.array([[0.0, 0.0, -800.0], [0.6, -0.4, -1300.0], [0.9, 0.9, -700.0], [-0.5, 0.8, -2500.0]], np.float32)
PROBE = dict(ks=21, spp=4096, param_list=[0.78, 1.44, 0.3, 0.5, "l"], seed=1)


def _bundle(ray):
    o, d = ray.o.detach().double(), ray.d.detach().double()
    return [t.numpy().copy() for t in (o[..., 0], o[..., 1], d[..., 0], d[..., 1], d[..., 2], ray.ra.detach().double())]


class Float64Sensor:
    """lens.d_sensor = s (a float64 leaf) for one psf_diff call; trace2sensor casts the traced bundle to float64 before
    it propagates; psf_center optionally without no_grad.  Records the bundles trace2sensor returned, in call order
    (psf_diff: the primary bundle, then the chief rays)."""

    def __init__(self, lens, s, centre_in_graph):
        self.lens, self.s, self.centre_in_graph, self.bundles = lens, s, centre_in_graph, []

    def __enter__(self):
        lens, rec = self.lens, self
        self._old = lens.d_sensor
        lens.d_sensor = self.s

        def trace2sensor(ray, record=False, ignore_invalid=False):
            with torch.no_grad():
                ray, _, _ = lens.trace(ray)
            ray.o, ray.d, ray.ra = ray.o.double(), ray.d.double(), ray.ra.double()
            ray = ray.propagate_to(lens.d_sensor)
            rec.bundles.append(_bundle(ray))
            return ray

        def centre(point, method="chief_ray"):
            assert method == "chief_ray"
            with torch.no_grad():
                ray = lens.sample_from_points(point, spp=ref_optics.GEO_SPP, shrink_pupil=True)
            ray = lens.trace2sensor(ray)
            weight = ray.ra.unsqueeze(-1)
            mean = (ray.o * weight).sum(0) / weight.sum(0).add(ref_optics.EPSILON)
            return -mean[..., :2]
        lens.trace2sensor = trace2sensor
        if self.centre_in_graph:
            lens.psf_center = centre
        return self

    def __exit__(self, *exc):
        self.lens.d_sensor = self._old
        del self.lens.trace2sensor
        if self.centre_in_graph:
            del self.lens.psf_center


def run(lens, points, r, direct, center, G, centre_in_graph, ks=KS, spp=SPP, seed=SEED, dp=DP, square=False):
    """One psf_diff call + backward with loss = sum(G psf) (+ sum(psf^2) with square) -> dict."""
    s = torch.tensor(float(lens.d_sensor), dtype=torch.float64, requires_grad=True)
    gg.set_seed(seed)
    with Float64Sensor(lens, s, centre_in_graph) as rec, dg.Splat64(cast=True) as sp:
        psf = lens.psf_diff(points=torch.tensor(points), ks=ks, spp=spp, center=center,
                            param_list=[*dp, r, direct])
    loss = (torch.from_numpy(G).to(psf.dtype) * psf).sum()
    if square:
        loss = loss + (psf ** 2).sum()
    loss.backward()
    return dict(s0=float(s.detach()), grad=float(s.grad), loss=float(loss.detach()), psf=psf.detach().numpy(), rays=rec.bundles[0],
                chief=rec.bundles[1] if center else None, centre=sp.center.astype(np.float64))


def probe_points(lens):
    pts = PROBE_POINTS.copy()
    pts[:, 2] += np.float32(lens.d_sensor)
    return pts


if __name__ == "__main__":
    lens = gg.build_lens("rf50mm")
    rng = np.random.default_rng(SEED)
    for r, direct, center in CASES:
        G = rng.standard_normal((len(POINTS), KS, KS)).astype(np.float32)
        for in_graph in ((False, True) if center else (False,)):
            out = run(lens, POINTS, r, direct, center, G, in_graph)
            print(f"r={r} direct={direct} center={center} centre in graph={in_graph}: dloss/ds = {out['grad']:+.9e}")
