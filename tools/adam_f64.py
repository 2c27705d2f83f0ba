"""The calibration problem of tests/test_gpu_trace_grad.py::test_adam_recovers_a_perturbed_air_gap_and_curvature in float64
on the CPU: where that test's loss ratio and shrink factors come from.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py).  The same 12 points, pupil
samples (problem() below is what the GPU test calls), ks, dual-pixel parameters, perturbation, Adam step lengths and
number of steps.  Per step the reference's float64 trace decides which rays are alive and how many Newton trips run
(tools/gen_trace_grad.py); the PSFs and their gradient are the float64 restatement's (tests/trace_f64.py with
splat_f64), max-normalised as psf_lr does.  One simplification: the entrance pupil's plane and the pinhole scale stay
those of the true lens, where the library recomputes them for every theta; the shift is second order in a 0.03 mm
change of one air gap.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, SPP, N_POINTS, STEPS = 31, 8192, 12, 12
DP = (0.78, 1.44, 0.3, 0.5)
D_SURFACE, C_SURFACE, D_OFF, C_FACTOR = 2, 4, 0.03, 1.004
LR_D, LR_C_REL = 2e-3, 2e-4


def problem(pupil_r):
    """(points [N, 3], (x2, y2) [SPP]): the field points and the pupil samples, drawn on the CPU as sample_from_points does."""
    g = torch.Generator().manual_seed(9)
    xy = (torch.rand(N_POINTS, 2, generator=g) * 2 - 1) * 0.7
    z = -3000.0 + 2200.0 * torch.rand(N_POINTS, 1, generator=g)
    ang = torch.rand(SPP, generator=g) * 2 * np.pi
    rad = torch.sqrt(torch.rand(SPP, generator=g) * float(pupil_r) ** 2)
    return torch.cat((xy, z), 1), (rad * torch.cos(ang), rad * torch.sin(ang))


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_trace_grad as gen
    import trace_f64 as T
    from conftest import make_lens
    from splat_f64 import max_normalise
    ref = gen.gg.build_lens("rf50mm")
    lens = make_lens("rf50mm", "cpu")
    pz, pr = ref.entrance_pupil()
    pts, (x2, y2) = problem(pr)
    scale = ref.calc_scale_pinhole(pts[:, 2])
    src = torch.stack((pts[:, 0] * scale * ref.sensor_size[1] / 2, pts[:, 1] * scale * ref.sensor_size[0] / 2, pts[:, 2]), -1)
    cen = torch.stack((pts[:, 0] * (ref.sensor_size[1] / 2), pts[:, 1] * (ref.sensor_size[0] / 2)), -1).double()
    aim = torch.stack((x2, y2, torch.full_like(x2, float(pz))), -1)
    o = src.unsqueeze(1).expand(N_POINTS, SPP, 3).reshape(-1, 3).contiguous()                      # point-major
    d = torch.nn.functional.normalize(aim.double().unsqueeze(0) - src.double().unsqueeze(1), dim=-1).reshape(-1, 3)
    table = T.lens_table(lens, 0.589)
    truth = lens.surface_parameters().double()
    dp = tuple(torch.tensor(v, dtype=torch.float64) for v in DP[:3]) + (DP[3],)

    def psfs(theta):
        with torch.no_grad():
            ref.surfaces[D_SURFACE].d = torch.tensor(float(theta[D_SURFACE, 0]))
            ref.surfaces[C_SURFACE].c = torch.tensor(float(theta[C_SURFACE, 1]))
        _, live, trips = gen._run(ref, o, d, torch.float64, lambda ray, lv: (ray.o * 0).sum())
        live = torch.from_numpy(live).reshape(N_POINTS, SPP)
        # a dead ray carries no weight: trace the point's first live ray in its place
        first = live.float().argmax(1, keepdim=True) + torch.arange(N_POINTS).unsqueeze(1) * SPP
        idx = torch.where(live, torch.arange(N_POINTS * SPP).reshape(N_POINTS, SPP), first).reshape(-1)
        L, R = T.psf_f64(o[idx].double(), d[idx], theta, table, trips, float(ref.d_sensor), SPP, N_POINTS, cen,
                         float(ref.pixel_size), KS, dp, ra=live.reshape(-1).float())
        return max_normalise(L), max_normalise(R)
    tL, tR = (t.detach() for t in psfs(truth))
    start = truth.clone()
    start[D_SURFACE, 0] += D_OFF
    start[C_SURFACE, 1] *= C_FACTOR
    d_par = start[D_SURFACE, 0].clone().requires_grad_()
    c_par = start[C_SURFACE, 1].clone().requires_grad_()
    opt = torch.optim.Adam([{"params": [d_par], "lr": LR_D}, {"params": [c_par], "lr": float(abs(truth[C_SURFACE, 1])) * LR_C_REL}])
    losses = []
    for _ in range(STEPS):
        theta = start.clone()
        theta[D_SURFACE, 0], theta[C_SURFACE, 1] = d_par, c_par
        L, R = psfs(theta)
        loss = ((L - tL) ** 2).mean() + ((R - tR) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("losses", " ".join(f"{v:.4e}" for v in losses))
    print(f"loss ratio last / first = {losses[-1] / losses[0]:.4f}")
    print(f"|d - truth| / start = {abs(float(d_par) - float(truth[D_SURFACE, 0])) / D_OFF:.4f}   "
          f"|c / truth - 1| / start = {abs(float(c_par) / float(truth[C_SURFACE, 1]) - 1) / (C_FACTOR - 1):.4f}")


if __name__ == "__main__":
    main()
