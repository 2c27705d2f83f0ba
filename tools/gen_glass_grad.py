"""The reference's own autograd gradients in the glass (n, V of every medium), for tests/test_glass_grad_cpu.py.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py); nothing it computes is
committed.  The counterpart of tools/gen_trace_grad.py, whose bundles, trip counting and lens construction it shares.
Per owned medium (Material.dispersion == 'naive': an 'n/V' string) one pair of float64 0-d leaves (n, V); both Material
objects of the medium (surfaces[j-1].mat2 and surfaces[j].mat1) get A, B = Material.nV_to_AB(n, V) of those leaves, so
that Material.ior returns a tensor and eta = mat1.ior / mat2.ior carries the graph through Aspheric._refract
(basics.py:316-362, surfaces.py:401-405, 633-669).  The leaves are float64 in the fp32 run as well: there the reference
holds its materials as Python floats, and what the run measures is the fp32 arithmetic of the rays.

cases(): the field corners of gen_trace_grad.CASES without the conic ones, each at 0.486, 0.589 and 0.656 um; the loss is
the fixed random linear form of the live rays' sensor-plane (o, d); float64 and fp32.  Recorded: the gradients
[K + 1, 2], the batch-wide Newton trip counts (counted as gen_trace_grad._run counts them) and the rays.
psf_cases(): the same chain through the reference's forward_integral, as gen_trace_grad.psf_cases, at two wavelengths.
main() prints the fp32-against-float64 spread over the sum of the per-ray magnitudes (tests/glass_f64.py with per-ray
eta leaves): the form of the GPU test's bound.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_trace_grad as gt  # noqa: E402  (imports the reference through oracle/_refimport.py)

gg, Ray, forward_integral = gt.gg, gt.Ray, gt.forward_integral
CASES = [(name, pt) for name, pt, conic in gt.CASES if conic is None]
WAVES = (0.486, 0.589, 0.656)
# (lens, field point, center, r, direct, wavelength)
PSF_CASES = [("rf50mm", (0.98, 0.98, -300.0), True, 0.5, "l", 0.486), ("rf50mm", (0.98, -0.98, -20000.0), False, 0.65, "r", 0.656),
             ("rf35mm", (0.98, 0.98, -300.0), False, 0.5, "l", 0.656), ("rf35mm", (-0.98, 0.98, -20000.0), True, 0.65, "r", 0.486)]
M, KS, DP = gt.M, gt.KS, gt.DP
_LENSES = {}


def lens_of(name):
    """One reference lens per name, reused: build_lens asserts on the run-to-run drift of the reference's pupil."""
    if name not in _LENSES:
        _LENSES[name] = gg.build_lens(name)
    return _LENSES[name]


def media(lens):
    """The K + 1 media of a reference lens as lists of their Material objects."""
    S = lens.surfaces
    return [[S[0].mat1]] + [[S[j - 1].mat2, S[j].mat1] for j in range(1, len(S))] + [[S[-1].mat2]]


def _run(lens, o, d, dtype, wvln, loss_of):
    """Trace the bundle at `wvln` with (n, V) leaves per owned medium, take loss_of(ray, live) and its gradient:
    (gradient [K + 1, 2], live [M], trips [K])."""
    med = media(lens)
    saved = [[(m, m.A, m.B) for m in objs] for objs in med]
    # the surfaces' own tensors in `dtype` for the call, as gen_trace_grad._run has them (fp32 ones would round c^2 (1 + k))
    params = [{n: getattr(s, n) for n in vars(s) if n in ("d", "c", "k") or n.startswith("ai")} for s in lens.surfaces]
    for s in lens.surfaces:
        gt._leaves(s, dtype)
    leaves = {}
    for j, objs in enumerate(med):
        if objs[0].dispersion == "naive":
            assert all((m.n, m.V) == (objs[0].n, objs[0].V) for m in objs)
            n = torch.tensor(float(objs[0].n), dtype=torch.float64, requires_grad=True)
            V = torch.tensor(float(objs[0].V), dtype=torch.float64, requires_grad=True)
            leaves[j] = (n, V)
            for m in objs:
                m.A, m.B = m.nV_to_AB(n, V)
    trips = [0] * len(lens.surfaces)
    cls = type(lens.surfaces[0])
    loose = cls._valid_loose

    def counted(self, x, y):
        trips[lens.surfaces.index(self)] += 1
        return loose(self, x, y)
    cls._valid_loose = counted
    try:
        try:
            ray = lens.trace2sensor(Ray(o.to(dtype), d.to(dtype), wvln=wvln, ra=torch.ones(o.shape[:-1], dtype=dtype), device="cpu"))
        finally:
            cls._valid_loose = loose
        live = ray.ra.detach() == 1
        loss_of(ray, live).backward()
        g = np.zeros((len(med), 2))
        for j, (n, V) in leaves.items():
            g[j] = (0.0 if n.grad is None else float(n.grad), 0.0 if V.grad is None else float(V.grad))
    finally:
        for objs in saved:
            for m, A, B in objs:
                m.A, m.B = A, B
        for s, sv in zip(lens.surfaces, params):
            for n, v in sv.items():
                setattr(s, n, v)
    return g, live.reshape(-1).numpy(), trips


def cases():
    out = []
    for i, (name, pt) in enumerate(CASES):
        lens = lens_of(name)
        for wvln in WAVES:
            gen = torch.Generator().manual_seed(400 + i)
            _, o, d = gt._bundle(lens, pt, gen)
            wo, wd = torch.randn(M, 3, generator=gen), torch.randn(M, 3, generator=gen)

            def run(keep, dtype):
                w1, w2 = wo[keep], wd[keep]
                linear = lambda ray, live: (ray.o * w1.to(dtype))[live].sum() + (ray.d * w2.to(dtype))[live].sum()
                return _run(lens, o[keep], d[keep], dtype, wvln, linear)
            every = np.ones(M, bool)
            _, live32, _ = run(every, torch.float32)
            _, live64, _ = run(every, torch.float64)
            keep = live32 & live64
            assert keep.mean() > 0.5, "most rays must reach the sensor"
            g64, live64, trips64 = run(keep, torch.float64)
            g32, live32, trips32 = run(keep, torch.float32)
            assert live64.all() and live32.all()
            out.append(dict(lens=name, conic=None, wvln=wvln, d_sensor=float(lens.d_sensor), trips=trips64, trips32=trips32,
                            o=o[keep].double().numpy(), d=d[keep].numpy(), wo=wo[keep].double().numpy(),
                            wd=wd[keep].double().numpy(), grad64=g64, grad32=g32))
    return out


def psf_cases():
    out = []
    for i, (name, pt, center, r, direct, wvln) in enumerate(PSF_CASES):
        lens = lens_of(name)
        gen = torch.Generator().manual_seed(500 + i)
        src, o, d = gt._bundle(lens, pt, gen)
        G = torch.randn(1, KS, KS, generator=gen, dtype=torch.float64)
        if center:
            torch.manual_seed(600 + i)
            cen = lens.psf_center(src).double()
        else:
            cen = torch.tensor([[pt[0] * lens.sensor_size[1] / 2, pt[1] * lens.sensor_size[0] / 2]], dtype=torch.float64)
        dp = [torch.tensor(v, dtype=torch.float64) for v in DP]

        def psf_loss(ray, live):
            assert bool(live.all())
            torch.set_default_dtype(torch.float64)          # the grids the splat allocates and r, as gen_trace_grad.py
            try:
                return (G * forward_integral(ray, lens.pixel_size, KS, pointc_ref=cen, param_list=[*dp, r, direct])).sum()
            finally:
                torch.set_default_dtype(torch.float32)
        _, live, _ = _run(lens, o, d, torch.float64, wvln, lambda ray, lv: (ray.o * 0).sum())
        assert live.mean() > 0.5, "most rays must reach the sensor"
        o, d = o[live].unsqueeze(1), d[live].unsqueeze(1)                       # [spp, N = 1, 3]
        g64, _, trips = _run(lens, o, d, torch.float64, wvln, psf_loss)
        assert np.abs(g64).max() > 0
        out.append(dict(lens=name, conic=None, wvln=wvln, d_sensor=float(lens.d_sensor), trips=trips, center=cen.numpy(),
                        ps=float(lens.pixel_size), ks=KS, dp=(*DP, r), direct=direct, G=G.numpy(),
                        o=o[:, 0].double().numpy(), d=d[:, 0].numpy(), grad64=g64))
    return out


def normalised_spread(case):
    """max over the owned (medium, column) of |g32 - g64| / sum over rays |per-ray term|: the per-ray terms from the
    float64 restatement with one eta leaf per ray and surface, taken to (n, V) by the Jacobian of eta in the glass."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import glass_f64 as G
    import trace_f64 as T
    from conftest import make_lens
    lens = make_lens(case["lens"], "cpu")
    K, m = len(lens.surfaces), len(case["o"])
    glass = lens.glass_parameters()
    J = torch.autograd.functional.jacobian(lambda g: G.eta(g, lens, case["wvln"]), glass)          # [K, K + 1, 2]
    etas = [G.eta(glass, lens, case["wvln"])[k].expand(m, 1).clone().requires_grad_() for k in range(K)]
    so, sd = G.trace_f64(torch.from_numpy(case["o"]), torch.from_numpy(case["d"]), lens.surface_parameters().double(),
                         G.glass_table(lens, case["wvln"], etas), case["trips"], case["d_sensor"])
    ((so * torch.from_numpy(case["wo"])).sum() + (sd * torch.from_numpy(case["wd"])).sum()).backward()
    per_ray = torch.stack([e.grad.reshape(-1) if e.grad is not None else torch.zeros(m, dtype=torch.float64) for e in etas], -1)  # [m, K]
    mag = torch.einsum("mk,kjc->mjc", per_ray, J).abs().sum(0).numpy()
    own = lens.glass_owned().numpy()
    return float((np.abs(case["grad32"] - case["grad64"])[own] / mag[own]).max())


def main():
    worst = 0.0
    for c in cases():
        s = normalised_spread(c)
        worst = max(worst, s)
        print(f"{c['lens']} {c['wvln']} um point {c['o'][0].round(1).tolist()}: {len(c['o'])} live rays, trips {c['trips']} "
              f"(fp32 {c['trips32']}), max |g64| = {np.abs(c['grad64']).max():.3e}, max |g32 - g64| / sum |per-ray terms| = {s:.3e}")
    print(f"largest normalised fp32-against-float64 spread: {worst:.3e}")
    for c in psf_cases():
        print(f"psf {c['lens']} {c['wvln']} um center {c['center'].tolist()} r {c['dp'][3]} {c['direct']}: {len(c['o'])} live rays, "
              f"trips {c['trips']}, max |g64| = {np.abs(c['grad64']).max():.3e}")


if __name__ == "__main__":
    main()
