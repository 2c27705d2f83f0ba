"""The reference's own autograd gradients in the surface parameters, for tests/test_trace_grad_cpu.py.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py); nothing it computes is
committed.  For every case a bundle from one field point to random pupil points is traced to the sensor by the reference's
Lensgroup.trace2sensor (deeplens/optics.py:638-664) with the surfaces' d, c, k, ai* as leaves (Aspheric.activate_grad's
set, surfaces.py:837-860).

cases(): the loss is a fixed random linear form of the live rays' sensor-plane (o, d); once in fp32 and once with the rays
and the leaves cast to float64.  Recorded: the float64 gradient [K, 3 + 8] and the fp32 one (main() prints their spread
over the largest entry and, per parameter, over the sum of the per-ray magnitudes, which the float64 restatement
supplies: the form of the GPU test's bound); the batch-wide Newton trip counts (one _valid_loose call per trip) and the
rays, so that trace_f64 can replay the case.  Field corners of rf50mm and rf35mm at 0.3 m and at 20 m, and the same
with a conic constant k != 0 on the aspheres (CONIC: one above and, on rf50mm, one below -1, the branch without the
Newton mask), which makes k a parameter of theirs.

psf_cases(): the PSF level.  The traced float64 bundle goes on through the reference's forward_integral
(monte_carlo.py:9-68, psf_diff's graph without its normalisation) with float64 grids, and the loss is sum(G * psf) for
a fixed G: both centre rules (the chief-ray centre of psf_center, the pinhole centre of optics.py:973-976), both area
models (r = 0.5 and 0.65), both directions, a field corner at 0.3 m and at 20 m, both lenses, and one with CONIC.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  (imports the reference through _refimport)

Ray = gg.deeplens.basics.Ray
forward_integral = gg.ref_optics.forward_integral
CONIC = {"rf50mm": {8: -1.3, 9: 0.4}, "rf35mm": {10: 0.5}}
# (lens, normalised field point, conic constants on the aspheres or None)
CASES = [("rf50mm", (0.98, 0.98, -300.0), None), ("rf50mm", (0.98, -0.98, -20000.0), None),
         ("rf35mm", (0.98, 0.98, -300.0), None), ("rf35mm", (-0.98, 0.98, -20000.0), None),
         ("rf50mm", (0.98, 0.98, -300.0), CONIC["rf50mm"]), ("rf35mm", (-0.98, 0.98, -20000.0), CONIC["rf35mm"])]
# (lens, field point, conic, center, r, direct)
PSF_CASES = [("rf50mm", (0.98, 0.98, -300.0), None, True, 0.5, "l"), ("rf50mm", (0.98, 0.98, -300.0), None, False, 0.65, "r"),
             ("rf50mm", (0.98, -0.98, -20000.0), None, False, 0.5, "r"), ("rf50mm", (0.98, -0.98, -20000.0), None, True, 0.65, "l"),
             ("rf35mm", (0.98, 0.98, -300.0), None, False, 0.5, "l"), ("rf35mm", (0.98, 0.98, -300.0), None, True, 0.65, "r"),
             ("rf35mm", (-0.98, 0.98, -20000.0), None, True, 0.5, "r"), ("rf35mm", (-0.98, 0.98, -20000.0), None, False, 0.65, "l"),
             ("rf50mm", (0.98, 0.98, -300.0), CONIC["rf50mm"], True, 0.65, "l")]
M, MAX_AI, WVLN = 512, 8, 0.589
KS = 65              # at 0.3 m the pinhole centre of a corner lies up to 40 pixels from the spot: a window that still holds it
DP = (0.78, 1.44, 0.3)


def _leaves(s, dtype):
    """The surface's parameter tensors recast as leaves of `dtype`: {column: tensor}."""
    out = {}
    for col, name in [(0, "d"), (1, "c"), (2, "k")] + [(3 + i, f"ai{2 * i + 2}") for i in range(s.ai_degree if s.ai is not None else 0)]:
        t = getattr(s, name).detach().to(dtype).clone().requires_grad_()
        setattr(s, name, t)
        out[col] = t
    return out


def _run(lens, o, d, dtype, loss_of, conic=None):
    """Trace the bundle with leaves of `dtype` (the aspheres' k set to `conic` for the call), take loss_of(ray, live)
    and its gradient: (gradient [K, 3 + MAX_AI], live [M], trips [K])."""
    saved = [{n: getattr(s, n) for n in vars(s) if n in ("d", "c", "k") or n.startswith("ai")} for s in lens.surfaces]
    for i, v in (conic or {}).items():
        lens.surfaces[i].k = torch.Tensor([v])
    leaves = [_leaves(s, dtype) for s in lens.surfaces]
    trips = [0] * len(lens.surfaces)
    cls = type(lens.surfaces[0])
    loose = cls._valid_loose

    def counted(self, x, y):
        trips[lens.surfaces.index(self)] += 1
        return loose(self, x, y)
    cls._valid_loose = counted
    try:
        ray = lens.trace2sensor(Ray(o.to(dtype), d.to(dtype), wvln=WVLN, ra=torch.ones(o.shape[:-1], dtype=dtype), device="cpu"))
    finally:
        cls._valid_loose = loose
    live = ray.ra.detach() == 1
    try:
        loss_of(ray, live).backward()
        g = np.zeros((len(lens.surfaces), 3 + MAX_AI))
        for k, lv in enumerate(leaves):
            for col, t in lv.items():
                g[k, col] = 0.0 if t.grad is None else float(t.grad)
    finally:
        for s, sv in zip(lens.surfaces, saved):
            for n, v in sv.items():
                setattr(s, n, v)
    return g, live.reshape(-1).numpy(), trips


def _bundle(lens, pt, gen):
    """M rays from the field point to random points of 0.8 of the entrance pupil: (source [1, 3], o [M, 3], d [M, 3])."""
    scale = lens.calc_scale_pinhole(pt[2])
    src = torch.tensor([[pt[0] * scale * lens.sensor_size[1] / 2, pt[1] * scale * lens.sensor_size[0] / 2, pt[2]]])
    pz, pr = lens.entrance_pupil()
    rad = torch.rand(M, generator=gen).sqrt() * float(pr) * 0.8
    ang = torch.rand(M, generator=gen) * 2 * np.pi
    aim = torch.stack((rad * ang.cos(), rad * ang.sin(), torch.full((M,), float(pz))), -1)
    o = src.expand(M, 3).contiguous()
    return src, o, torch.nn.functional.normalize(aim.double() - o.double(), dim=-1)     # float64 unit vectors: Ray() renormalises


def cases():
    out, lenses = [], {}
    for i, (name, pt, conic) in enumerate(CASES):
        lens = lenses.setdefault(name, gg.build_lens(name))
        gen = torch.Generator().manual_seed(100 + i)
        _, o, d = _bundle(lens, pt, gen)
        wo, wd = torch.randn(M, 3, generator=gen), torch.randn(M, 3, generator=gen)

        def run(keep, dtype):
            w1, w2 = wo[keep], wd[keep]
            linear = lambda ray, live: (ray.o * w1.to(dtype))[live].sum() + (ray.d * w2.to(dtype))[live].sum()
            return _run(lens, o[keep], d[keep], dtype, linear, conic)
        every = np.ones(M, bool)
        g32, live32, trips32 = run(every, torch.float32)
        g64, live64, trips64 = run(every, torch.float64)
        keep = live32 & live64
        assert keep.mean() > 0.5, "most rays must reach the sensor"
        if not keep.all():
            g64, live64, trips64 = run(keep, torch.float64)
            g32, live32, trips32 = run(keep, torch.float32)
            assert live64.all() and live32.all()
        out.append(dict(lens=name, conic=conic, wvln=WVLN, d_sensor=float(lens.d_sensor), trips=trips64, trips32=trips32,
                        o=o[keep].double().numpy(), d=d[keep].numpy(), wo=wo[keep].double().numpy(),
                        wd=wd[keep].double().numpy(), grad64=g64, grad32=g32))
    return out


def psf_cases():
    out, lenses = [], {}
    for i, (name, pt, conic, center, r, direct) in enumerate(PSF_CASES):
        lens = lenses.setdefault(name, gg.build_lens(name))
        gen = torch.Generator().manual_seed(200 + i)
        src, o, d = _bundle(lens, pt, gen)
        G = torch.randn(1, KS, KS, generator=gen, dtype=torch.float64)
        if center:
            torch.manual_seed(300 + i)
            cen = lens.psf_center(src).double()
        else:
            cen = torch.tensor([[pt[0] * lens.sensor_size[1] / 2, pt[1] * lens.sensor_size[0] / 2]], dtype=torch.float64)
        dp = [torch.tensor(v, dtype=torch.float64) for v in DP]

        def psf_loss(ray, live):
            assert bool(live.all())
            torch.set_default_dtype(torch.float64)          # the grids the splat allocates and r, as gen_golden_dp_grad.py
            try:
                return (G * forward_integral(ray, lens.pixel_size, KS, pointc_ref=cen, param_list=[*dp, r, direct])).sum()
            finally:
                torch.set_default_dtype(torch.float32)
        _, live, _ = _run(lens, o, d, torch.float64, lambda ray, lv: (ray.o * 0).sum(), conic)
        assert live.mean() > 0.5, "most rays must reach the sensor"
        o, d = o[live].unsqueeze(1), d[live].unsqueeze(1)                       # [spp, N = 1, 3]
        g64, _, trips = _run(lens, o, d, torch.float64, psf_loss, conic)
        assert np.abs(g64).max() > 0
        out.append(dict(lens=name, conic=conic, wvln=WVLN, d_sensor=float(lens.d_sensor), trips=trips, center=cen.numpy(),
                        ps=float(lens.pixel_size), ks=KS, dp=(*DP, r), direct=direct, G=G.numpy(),
                        o=o[:, 0].double().numpy(), d=d[:, 0].numpy(), grad64=g64))
    return out


def normalised_spread(case):
    """max over the owned columns (the stop's d apart: its terms vanish) of |g32 - g64| / sum over rays |per-ray term|,
    the per-ray terms from the float64 restatement (tests/trace_f64.py) with one parameter leaf per ray."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import trace_f64 as T
    from conftest import make_lens
    lens = T.with_conic(make_lens(case["lens"], "cpu"), case["conic"])
    th = lens.surface_parameters().double().unsqueeze(0).expand(len(case["o"]), -1, -1).clone().requires_grad_()
    so, sd = T.trace_f64(torch.from_numpy(case["o"]), torch.from_numpy(case["d"]), th, T.lens_table(lens, case["wvln"]),
                         case["trips"], case["d_sensor"])
    ((so * torch.from_numpy(case["wo"])).sum() + (sd * torch.from_numpy(case["wd"])).sum()).backward()
    mag = th.grad.abs().sum(0).numpy()
    own = np.stack([s.owned_columns() for s in lens.surfaces])
    own[lens.aper_idx] = False
    return float((np.abs(case["grad32"] - case["grad64"])[own] / mag[own]).max())


def main():
    for c in cases():
        spread = np.abs(c["grad32"] - c["grad64"]).max() / np.abs(c["grad64"]).max()
        print(f"{c['lens']} conic {c['conic']}: {len(c['o'])} live rays, trips {c['trips']} (fp32 {c['trips32']}), "
              f"max |g32 - g64| / max |g64| = {spread:.3e}, max |g32 - g64| / sum |per-ray terms| = {normalised_spread(c):.3e}")


    for c in psf_cases():
        print(f"psf {c['lens']} conic {c['conic']} center {c['center'].tolist()} r {c['dp'][3]} {c['direct']}: {len(c['o'])} live rays, "
              f"trips {c['trips']}, max |g64| = {np.abs(c['grad64']).max():.3e}")


if __name__ == "__main__":
    main()
