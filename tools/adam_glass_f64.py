"""The calibration problem of tests/test_gpu_glass_grad.py::test_adam_recovers_a_perturbed_index in float64 on the CPU:
where that test's loss ratio and shrink factor come from.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py).  Built like tools/adam_f64.py,
whose problem() (12 points, 8192 pupil samples, ks 31, pinhole centres) it shares: PSFs of the true rf50mm as the target,
n of its first element (medium 1) starts N_OFF too high, Adam for 12 steps.  Per step the reference's float64 trace
with that glass decides which rays are alive and how many Newton trips run (tools/gen_glass_grad.py); the PSFs and their
gradient are the float64 restatement's (tests/glass_f64.py with splat_f64), max-normalised as psf_lr does.  The same
simplification as adam_f64.py: the entrance pupil's plane and the pinhole scale stay those of the true lens.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from adam_f64 import DP, KS, N_POINTS, SPP, STEPS, problem  # noqa: E402,F401  (importing it needs no reference)

MEDIUM, N_OFF, LR_N, WVLN = 1, 2e-3, 1.3e-4, 0.589


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen_glass_grad as gen
    import glass_f64 as G
    from conftest import make_lens
    from splat_f64 import max_normalise, splat_f64
    ref = gen.lens_of("rf50mm")
    lens = make_lens("rf50mm", "cpu")
    pz, pr = ref.entrance_pupil()
    pts, (x2, y2) = problem(pr)
    scale = ref.calc_scale_pinhole(pts[:, 2])
    src = torch.stack((pts[:, 0] * scale * ref.sensor_size[1] / 2, pts[:, 1] * scale * ref.sensor_size[0] / 2, pts[:, 2]), -1)
    cen = torch.stack((pts[:, 0] * (ref.sensor_size[1] / 2), pts[:, 1] * (ref.sensor_size[0] / 2)), -1).double()
    aim = torch.stack((x2, y2, torch.full_like(x2, float(pz))), -1)
    o = src.unsqueeze(1).expand(N_POINTS, SPP, 3).reshape(-1, 3).contiguous()                      # point-major
    d = torch.nn.functional.normalize(aim.double().unsqueeze(0) - src.double().unsqueeze(1), dim=-1).reshape(-1, 3)
    theta = lens.surface_parameters().double()
    truth = lens.glass_parameters()
    dp = tuple(torch.tensor(v, dtype=torch.float64) for v in DP[:3]) + (DP[3],)
    sn = lambda v: v.reshape(N_POINTS, SPP).t()

    def psfs(glass):
        objs = gen.media(ref)[MEDIUM]
        old = [m.n for m in objs]
        for m in objs:
            m.n = float(glass[MEDIUM, 0])
        try:
            _, live, trips = gen._run(ref, o, d, torch.float64, WVLN, lambda ray, lv: (ray.o * 0).sum())
        finally:
            for m, n in zip(objs, old):
                m.n = n
        live = torch.from_numpy(live).reshape(N_POINTS, SPP)
        # a dead ray carries no weight: trace the point's first live ray in its place
        first = live.float().argmax(1, keepdim=True) + torch.arange(N_POINTS).unsqueeze(1) * SPP
        idx = torch.where(live, torch.arange(N_POINTS * SPP).reshape(N_POINTS, SPP), first).reshape(-1)
        table = G.glass_table(lens, WVLN, list(G.eta(glass, lens, WVLN)))
        so, sd = G.trace_f64(o[idx].double(), d[idx], theta, table, trips, float(ref.d_sensor))
        L, R = splat_f64(sn(so[:, 0]), sn(so[:, 1]), sn(sd[:, 0]), sn(sd[:, 2]), sn(live.reshape(-1).float()), cen,
                         float(ref.pixel_size), KS, *dp)
        return max_normalise(L), max_normalise(R)
    tL, tR = (t.detach() for t in psfs(truth))
    n_par = (truth[MEDIUM, 0] + N_OFF).clone().requires_grad_()
    opt = torch.optim.Adam([n_par], lr=LR_N)
    losses = []
    for _ in range(STEPS):
        glass = truth.clone()
        glass[MEDIUM, 0] = n_par
        L, R = psfs(glass)
        loss = ((L - tL) ** 2).mean() + ((R - tR) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("losses", " ".join(f"{v:.4e}" for v in losses))
    print("monotone", all(b < a for a, b in zip(losses, losses[1:])))
    print(f"loss ratio last / first = {losses[-1] / losses[0]:.4f}")
    print(f"|n - truth| / start = {abs(float(n_par) - float(truth[MEDIUM, 0])) / N_OFF:.4f}")


if __name__ == "__main__":
    main()
