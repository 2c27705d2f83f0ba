"""The reference's own autograd gradients in the OBJECT POINTS, for tests/test_point_grad_cpu.py.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py); nothing it computes is
committed.  For every case the body of Lensgroup.psf_diff (deeplens/optics.py:956-976, without its normalisation) runs
with `points` [1, 3] as a leaf and with the two @torch.no_grad() samplers replaced by their undecorated functions
(Lensgroup.sample_from_points.__wrapped__, Lensgroup.psf_center.__wrapped__), so that the rays and, with center=True,
the chief-ray centre are in the graph -- and with calc_scale_pinhole.__wrapped__: the reference decorates the pinhole
scale s = -z tan(hfov) / r_last with no_grad as well (optics.py:1301), which would cut the depth out of point_obj.xy, and
the derivative wanted is that of the forward arithmetic (the reference's own central differences in the depth agree with
the undecorated graph, not with the decorated one); the loss is sum(G * forward_integral(...)) for a fixed G.  The four pupil draws
(torch.rand at optics.py:483-484, primary then chief) are fixed fp32 tensors handed out in order, and the entrance pupil
(z, r), shrunk and not, is computed once in fp32 and held: both are constants of the derivative.  Once in fp32 and once
in float64 (points, surface tensors and torch's default dtype; the draws and so the pupil points stay the same fp32
values).  Pupil samples whose ray dies in either precision are dropped from both runs (N = 1: a dead ray has weight 0,
so the sums are those of the full bundle), which leaves a bundle that is alive throughout, as the float64 restatement
needs it.

Cases: the rows of tools/gen_trace_grad.py's PSF_CASES without a conic constant -- both centre rules, r = 0.5 and 0.65,
both directions, both lenses, a field corner at 0.3 m and at 20 m each, where rays die at the stop and the asphere.

main() prints, per case and component (x, y, depth of the normalised point), |g32 - g64| over the sum of the per-ray
magnitudes |term| (the float64 restatement's, tests/point_f64.py, with one copy of the point per ray): the form of the
GPU test's bound.
"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_trace_grad as gen  # noqa: E402  (imports the reference through oracle/_refimport)

gg = gen.gg
forward_integral = gen.forward_integral
PSF_CASES = [c for c in gen.PSF_CASES if c[2] is None]
SPP, WVLN, KS, DP = gen.M, gen.WVLN, gen.KS, gen.DP
CHIEF_SPP = 2048          # the reference's GEO_SPP (psf_center, optics.py:900)


@contextlib.contextmanager
def _in_graph(lens, dtype, draws, pupils, log):
    """The samplers and the pinhole scale without no_grad, torch.rand handing out `draws` in order, the pupils held, the surfaces' tensors and
    torch's default dtype cast to `dtype`; every trace2sensor call appends (ra, Newton trips) to `log`."""
    cls = type(lens)
    saved_methods = (cls.sample_from_points, cls.psf_center, cls.calc_scale_pinhole)
    saved = [{n: getattr(s, n) for n in vars(s) if n in ("d", "c", "k") or n.startswith("ai")} for s in lens.surfaces]
    scls = type(lens.surfaces[0])
    loose, rand, default = scls._valid_loose, torch.rand, torch.get_default_dtype()
    trips = [0] * len(lens.surfaces)
    queue = list(draws)

    def counted(self, x, y):
        trips[lens.surfaces.index(self)] += 1
        return loose(self, x, y)

    def traced(ray, *a, **k):
        trips[:] = [0] * len(trips)
        out = cls.trace2sensor(lens, ray, *a, **k)
        log.append((out.ra.detach().clone(), list(trips)))
        return out

    def fixed_rand(n, *a, **k):
        t = queue.pop(0)
        assert t.shape == (n,), (t.shape, n)
        return t.clone()
    cls.sample_from_points = cls.sample_from_points.__wrapped__
    cls.psf_center = cls.psf_center.__wrapped__
    cls.calc_scale_pinhole = cls.calc_scale_pinhole.__wrapped__
    scls._valid_loose = counted
    torch.rand = fixed_rand
    lens.trace2sensor = traced
    lens.entrance_pupil = lambda *a, **k: pupils[bool(k.get("shrink_pupil", False))]
    for s in lens.surfaces:
        for n, v in list(vars(s).items()):
            if (n in ("d", "c", "k") or n.startswith("ai")) and torch.is_tensor(v):
                setattr(s, n, v.detach().to(dtype))
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(default)
        torch.rand = rand
        scls._valid_loose = loose
        cls.sample_from_points, cls.psf_center, cls.calc_scale_pinhole = saved_methods
        del lens.trace2sensor, lens.entrance_pupil
        for s, sv in zip(lens.surfaces, saved):
            for n, v in sv.items():
                setattr(s, n, v)


def _loss(lens, points, center, r, direct, spp, G, dtype):
    """psf_diff's body, optics.py:956-976, and sum(G * psf)."""
    depth = points[:, 2]
    scale = lens.calc_scale_pinhole(depth)
    point_obj = points.clone()
    point_obj[..., 0] = points[..., 0] * scale * lens.sensor_size[1] / 2
    point_obj[..., 1] = points[..., 1] * scale * lens.sensor_size[0] / 2
    ray = lens.sample_from_points(o=point_obj, spp=spp, wvln=WVLN)
    ray = lens.trace2sensor(ray)
    if center:
        ref = lens.psf_center(point_obj)
    else:
        ref = points.clone()[:, :2]
        ref[:, 0] *= lens.sensor_size[1] / 2
        ref[:, 1] *= lens.sensor_size[0] / 2
    dp = [torch.tensor(v, dtype=dtype) for v in DP]
    psf = forward_integral(ray, ps=lens.pixel_size, ks=KS, pointc_ref=ref, param_list=[*dp, r, direct])
    return (G.to(dtype) * psf).sum(), ref.detach()


def _run(lens, pt, dtype, center, r, direct, draws, pupils, G, backward=True):
    """-> (gradient [3] in the normalised point or None, [(ra, trips)] of the primary and the chief trace, the centre)."""
    points = torch.tensor([list(pt)], dtype=dtype, requires_grad=True)
    log = []
    with _in_graph(lens, dtype, draws, pupils, log):
        loss, ref = _loss(lens, points, center, r, direct, draws[0].shape[0], G, dtype)
        if backward:
            loss.backward()
    return (points.grad[0].double().numpy() if backward else None), log, ref.double().numpy()


def pupil_points(u_theta, u_r2, pupil_r):
    """optics.py:483-486 on fixed fp32 uniforms."""
    theta = u_theta * 2 * np.pi
    rad = torch.sqrt(u_r2 * pupil_r ** 2)
    return rad * torch.cos(theta), rad * torch.sin(theta)


def cases():
    out, lenses = [], {}
    for i, (name, pt, _, center, r, direct) in enumerate(PSF_CASES):
        lens = lenses.setdefault(name, gg.build_lens(name))
        pupils = {False: tuple(float(v) for v in lens.entrance_pupil()),
                  True: tuple(float(v) for v in lens.entrance_pupil(shrink_pupil=True))}
        gen_ = torch.Generator().manual_seed(400 + i)
        draws = [torch.rand(SPP, generator=gen_), torch.rand(SPP, generator=gen_)]
        if center:
            draws += [torch.rand(CHIEF_SPP, generator=gen_), torch.rand(CHIEF_SPP, generator=gen_)]
        G = torch.randn(1, KS, KS, generator=gen_, dtype=torch.float64)
        # the pupil samples whose rays live in both precisions
        logs = [_run(lens, pt, dt, center, r, direct, draws, pupils, G, backward=False)[1] for dt in (torch.float32, torch.float64)]
        for b in range(len(draws) // 2):
            keep = (logs[0][b][0].reshape(-1) == 1) & (logs[1][b][0].reshape(-1) == 1)
            assert float(keep.float().mean()) > 0.5, "most rays must reach the sensor"
            draws[2 * b], draws[2 * b + 1] = draws[2 * b][keep], draws[2 * b + 1][keep]
        g32, log32, _ = _run(lens, pt, torch.float32, center, r, direct, draws, pupils, G)
        g64, log64, cen = _run(lens, pt, torch.float64, center, r, direct, draws, pupils, G)
        assert all(bool((ra == 1).all()) for ra, _ in log32 + log64)
        assert np.abs(g64).max() > 0 and np.isfinite(g64).all() and np.isfinite(g32).all()
        x2, y2 = pupil_points(draws[0], draws[1], pupils[False][1])
        case = dict(lens=name, point=np.asarray(pt, np.float64), center=center, r=r, direct=direct, wvln=WVLN,
                    d_sensor=float(lens.d_sensor), ps=float(lens.pixel_size), ks=KS, dp=(*DP, r), G=G.numpy(),
                    tan_hfov=float(np.tan(lens.hfov)), r_last=float(lens.r_last), sensor_w=float(lens.sensor_size[1]),
                    sensor_h=float(lens.sensor_size[0]), pupil_z=pupils[False][0], x2=x2.numpy(), y2=y2.numpy(),
                    trips=log64[0][1], trips32=log32[0][1], cen=cen, grad64=g64, grad32=g32)
        if center:
            xc, yc = pupil_points(draws[2], draws[3], pupils[True][1])
            case.update(pupil_z_c=pupils[True][0], xc=xc.numpy(), yc=yc.numpy(), trips_c=log64[1][1])
        out.append(case)
    return out


def chain(case, p_bar, absolute=False):
    """dLoss/d(normalised point) [3] from p_bar = dLoss/d(point_obj) [3] (optics.py:956-960); absolute=True: the same
    sum with every term's magnitude, for a p_bar that holds sums of magnitudes."""
    x, y, z = case["point"]
    hw, hh, q = case["sensor_w"] / 2, case["sensor_h"] / 2, case["tan_hfov"] / case["r_last"]
    s = -z * q
    if absolute:
        return np.array([p_bar[0] * abs(s) * hw, p_bar[1] * abs(s) * hh,
                         p_bar[2] + (abs(x) * hw * p_bar[0] + abs(y) * hh * p_bar[1]) * q])
    return np.array([p_bar[0] * s * hw, p_bar[1] * s * hh, p_bar[2] - (x * hw * p_bar[0] + y * hh * p_bar[1]) * q])


def restated(case, per_ray=False):
    """dLoss/d(points) [3] of the case by the float64 restatement (tests/point_f64.py).  per_ray=True: every ray
    (primary and chief) has its own copy of the object point as a leaf, -> (the gradient from the summed leaves through
    chain(), the sum of the per-ray magnitudes |term| through chain(absolute=True)): the normaliser of the spread."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import point_f64 as P
    import trace_f64 as T
    from conftest import make_lens
    lens = make_lens(case["lens"], "cpu")
    theta, table = lens.surface_parameters().double(), T.lens_table(lens, case["wvln"])
    scale = (case["tan_hfov"], case["r_last"], case["sensor_w"], case["sensor_h"])
    h, f, w = (torch.tensor(v, dtype=torch.float64) for v in case["dp"][:3])
    pts = torch.from_numpy(case["point"]).reshape(1, 3).clone().requires_grad_()
    leaves = []

    def bundle(x, y, pupil_z):
        x, y = torch.from_numpy(x), torch.from_numpy(y)
        po = P.object_points(pts, *scale).expand(len(x), 3)
        if per_ray:
            leaves.append(po.detach().clone().requires_grad_())
            po = leaves[-1]
        q = torch.stack((x.double(), y.double(), torch.full((len(x),), pupil_z, dtype=torch.float64)), -1)
        v = q - po
        return po, v / v.norm(dim=-1, keepdim=True)
    o, d = bundle(case["x2"], case["y2"], case["pupil_z"])
    if case["center"]:
        oc, dc = bundle(case["xc"], case["yc"], case["pupil_z_c"])
        so, _ = T.trace_f64(oc, dc, theta, table, case["trips_c"], case["d_sensor"])
        cen = -(so.sum(0) / (len(oc) + P.EPSILON))[:2].reshape(1, 2)
    else:
        # the pinhole centre (optics.py:973-976): one term per point, carried by `pts` itself
        cen = torch.stack((pts[:, 0] * case["sensor_w"] / 2, pts[:, 1] * case["sensor_h"] / 2), -1)
    L, R = T.psf_f64(o, d, theta, table, case["trips"], case["d_sensor"], len(o), 1, cen, case["ps"], case["ks"],
                     (h, f, w, case["dp"][3]), mask_dtype=torch.float64)
    (torch.from_numpy(case["G"]) * (R if case["direct"] == "r" else L)).sum().backward()
    if not per_ray:
        return pts.grad[0].numpy()
    own = pts.grad[0].numpy() if pts.grad is not None else np.zeros(3)
    total = chain(case, sum(l.grad.sum(0) for l in leaves).numpy()) + own
    mag = chain(case, sum(l.grad.abs().sum(0) for l in leaves).numpy(), absolute=True) + np.abs(own)
    return total, mag


def main():
    worst = 0.0
    for c in cases():
        total, mag = restated(c, per_ray=True)
        spread = np.abs(c["grad32"] - c["grad64"]) / mag
        rel = np.abs(total - c["grad64"]) / np.abs(c["grad64"]).max()
        worst = max(worst, float(spread.max()))
        print(f"{c['lens']} point {c['point'].tolist()} center {c['center']} r {c['r']} {c['direct']}: "
              f"{len(c['x2'])} primary rays, trips {c['trips']} (fp32 {c['trips32']}), g64 = {c['grad64']}, "
              f"|g32 - g64| / sum|per-ray terms| = {spread}, |restatement - g64| / max|g64| = {rel.max():.3e}")
    print(f"worst spread {worst:.3e}")


if __name__ == "__main__":
    main()
