"""The depth-by-descent problem of tests/test_gpu_point_grad.py::test_depth_by_descent in float64 on the CPU, and the
float64 error of the difference quotient of test_centre_jacobian_against_differences_of_the_fused_chief_centre: where
those tests' numbers come from.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py).  rf50mm with the sensor at
D_SENSOR, the position the reference's refocus(-1000) finds (printed by main(); every other lens scalar stays as it
is, as with psf_lr's d_sensor=).  Four points -- on axis, mid-field, a corner, one far behind the focus plane -- with
true depths between -700 and -3000 mm; fixed pupil samples (problem() below is what the GPU test calls), 4096 rays,
ks 31, chief-ray centres; the targets are the model's own sum-normalised L and R at the true depths; the depths start
8 % off; Adam on the four depths, one step length per point (a fraction of its starting depth, as the reference's
get_optimizer_params has one per parameter kind), falling linearly to 0.  Per step the reference's float64 trace
decides which rays are alive and how many Newton trips run (tools/gen_trace_grad.py); the PSFs, the chief-ray centres
and their gradient in the depth are the float64 restatement's (tests/point_f64.py).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, SPP, SC, STEPS = 31, 4096, 2048, 30
DP = (0.78, 1.44, 0.3, 0.5)
POINTS = [[0.0, 0.0, -1500.0], [0.5, -0.3, -800.0], [0.9, 0.9, -700.0], [-0.3, 0.6, -3000.0]]
START, LR_REL = 1.08, 6e-3
D_SENSOR = 62.07939910888672
# the results of main(): loss[-1] / loss[0] and max |z / truth - 1| after STEPS steps
RATIO, LEFT = 6.0351e-04, 4.8190e-03
# the centre's difference quotient in x at +-JAC_STEP against its own autograd, in float64: |quotient - jacobian| /
# max |jacobian| per point (x, y) at -1500 mm, lens as shipped
JAC_STEP = 0.01
JAC_ERR = {(0.0, 0.0): 5.934e-07, (0.7, 0.5): 1.591e-06}


def problem(pupil_r):
    """(points [N, 3], (x2, y2) [SPP], (xc, yc) [SC]): the points and the pupil samples, drawn on the CPU as
    sample_from_points does."""
    g = torch.Generator().manual_seed(19)

    def disc(n, radius):
        ang = torch.rand(n, generator=g) * 2 * np.pi
        rad = torch.sqrt(torch.rand(n, generator=g) * float(radius) ** 2)
        return rad * torch.cos(ang), rad * torch.sin(ang)
    return torch.tensor(POINTS), disc(SPP, pupil_r), disc(SC, pupil_r * 0.25)


def step_lengths(z_start):
    return [LR_REL * abs(float(z)) for z in z_start]


class Model:
    """The float64 restatement of psf_lr(center=True, normalize=False) / of the chief-ray centre as a function of the
    normalised points, the reference's float64 trace deciding the live rays and the trip counts of every call."""

    def __init__(self, d_sensor=None):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_trace_grad as gen
        import point_f64 as P
        import trace_f64 as T
        from conftest import make_lens
        self.gen, self.P, self.T = gen, P, T
        self.ref = gen.gg.build_lens("rf50mm")
        if d_sensor is not None:
            self.ref.d_sensor = d_sensor
        lens = make_lens("rf50mm", "cpu")
        self.theta, self.table = lens.surface_parameters().double(), T.lens_table(lens, 0.589)
        self.consts = (float(np.tan(self.ref.hfov)), float(self.ref.r_last), float(self.ref.sensor_size[1]),
                       float(self.ref.sensor_size[0]))
        self.pupil = tuple(float(v) for v in self.ref.entrance_pupil())
        self.ps = float(self.ref.pixel_size)

    def _alive(self, po, x, y):
        """(weights [N S], trips) of the bundle po -> pupil points, by the reference's float64 trace."""
        o, d = self.P.sample_rays(po.detach(), x, y, self.pupil[0])
        with torch.enable_grad():           # (_run takes a gradient, also when the caller does not record one)
            _, live, trips = self.gen._run(self.ref, o, d, torch.float64, lambda ray, lv: (ray.o * 0).sum())
        return torch.from_numpy(live).float(), trips

    def centre(self, pts, xc, yc):
        po = self.P.object_points(pts, *self.consts)
        ra, trips = self._alive(po, xc, yc)
        return self.P.centre(po, xc, yc, self.pupil[0], self.theta, self.table, trips, float(self.ref.d_sensor), ra)

    def psfs(self, pts, pxy, cxy):
        """Sum-normalised (L, R) [N, KS, KS]."""
        cen = self.centre(pts, *cxy)
        po = self.P.object_points(pts, *self.consts)
        ra, trips = self._alive(po, *pxy)
        dp = tuple(torch.tensor(v, dtype=torch.float64) for v in DP[:3]) + (DP[3],)
        L, R = self.P.psf_of_points(po, *pxy, self.pupil[0], self.theta, self.table, trips, float(self.ref.d_sensor), cen,
                                    self.ps, KS, dp, ra)
        return L / L.sum((-1, -2), keepdim=True), R / R.sum((-1, -2), keepdim=True)


def main():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_trace_grad as gen
    probe = gen.gg.build_lens("rf50mm")
    probe.refocus(-1000.0)
    print(f"refocus(-1000): d_sensor = {float(probe.d_sensor)!r}")
    # the quotient of the centre, lens as shipped
    m = Model()
    _, _, cxy = problem(m.pupil[1])
    for xy in ((0.0, 0.0), (0.7, 0.5)):
        p = torch.tensor([[xy[0], xy[1], -1500.0]], dtype=torch.float64)
        jac = []
        for comp in range(2):
            q = p.clone().requires_grad_()
            m.centre(q, *cxy)[0, comp].backward()
            jac.append(float(q.grad[0, 0]))
        lo, hi = p.clone(), p.clone()
        lo[0, 0] -= JAC_STEP
        hi[0, 0] += JAC_STEP
        with torch.no_grad():
            quot = (m.centre(hi, *cxy) - m.centre(lo, *cxy))[0] / (2 * JAC_STEP)
        jac = torch.tensor(jac, dtype=torch.float64)
        print(f"centre at {xy}: jacobian d c / d x = {jac.tolist()}, quotient at +-{JAC_STEP} = {quot.tolist()}, "
              f"|quotient - jacobian| / max |jacobian| = {float((quot - jac).abs().max() / jac.abs().max()):.3e}")
    m = Model(D_SENSOR)
    pts, pxy, cxy = problem(m.pupil[1])
    pts = pts.double()
    with torch.no_grad():
        tL, tR = m.psfs(pts, pxy, cxy)
    z0 = pts[:, 2] * START
    zs = [z.clone().requires_grad_() for z in z0]
    opt = torch.optim.Adam([{"params": [z], "lr": lr} for z, lr in zip(zs, step_lengths(z0))])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 - k / STEPS)
    losses = []
    for _ in range(STEPS):
        p = torch.cat((pts[:, :2], torch.stack(zs).unsqueeze(1)), 1)
        L, R = m.psfs(p, pxy, cxy)
        loss = ((L - tL) ** 2).sum() + ((R - tR) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss))
    z = torch.stack(zs).detach()
    print("losses", " ".join(f"{v:.4e}" for v in losses))
    print(f"loss ratio last / first = {losses[-1] / losses[0]:.4e}   z / truth - 1 = {(z / pts[:, 2] - 1).tolist()}   "
          f"max |z / truth - 1| = {float((z / pts[:, 2] - 1).abs().max()):.4e}")


if __name__ == "__main__":
    main()
