"""The focus-fitting problem of tests/test_gpu_focus_grad.py::test_adam_recovers_the_sensor_position in float64 on the
CPU: where that test's loss ratio and distance come from.

TEST INFRASTRUCTURE ONLY -- runs where the reference is available (oracle/_refimport.py).  The same points, pupil
samples (problem() below is what the GPU test calls), ks, dual-pixel parameters, offset, Adam step length and number
of steps.  The reference's fp32 trace supplies the bundles once, at the lens's own sensor position (the primary rays
and the green chief rays, tools/gen_focus_grad.py); from there on everything is the float64 restatement
tests/focus_f64.py: the rays move to the sensor position of the step analytically, the centre is the chief rays'
centroid there, the PSFs are max-normalised as psf_lr does.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, SPP, SC, STEPS = 21, 4096, 2048, 12
DP = (0.78, 1.44, 0.3, 0.5)
OFFSET, LR = 0.05, 8e-3
# the points whose PSFs stay inside a 21-pixel window (depth measured from the sensor: the caller adds d_sensor)
POINTS = [[0.0, 0.0, -800.0], [0.6, -0.4, -1300.0], [0.9, 0.9, -700.0], [-0.5, 0.8, -2500.0]]


def uniforms():
    """The four vectors of uniforms of one psf_diff call, in its order of drawing: primary (angle, radius^2), chief ray
    (angle, radius^2)."""
    g = torch.Generator().manual_seed(17)
    return [torch.rand(n, generator=g) for n in (SPP, SPP, SC, SC)]


def pupil_points(u_theta, u_r2, pupil_r):
    """sample_from_points' mapping of two vectors of uniforms to the pupil disc, in its fp32 CPU operations."""
    theta = u_theta * 2 * np.pi
    r = torch.sqrt(u_r2 * pupil_r ** 2)
    return r * torch.cos(theta), r * torch.sin(theta)


def problem(d_sensor, pupil_r):
    """(points [N, 3], (x2, y2) [SPP], (xc, yc) [SC]) for a lens whose sensor sits at d_sensor."""
    pts = torch.tensor(POINTS)
    pts[:, 2] += float(d_sensor)
    u = uniforms()
    return pts, pupil_points(u[0], u[1], pupil_r), pupil_points(u[2], u[3], pupil_r * 0.25)


def adam(psfs, start, truth):
    """STEPS Adam steps on the sensor position alone -> (losses, |t - truth| after the last step)."""
    t = torch.tensor(start, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t], lr=LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 - k / STEPS)      # the step length falls linearly to 0
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        loss = psfs(t)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
        sched.step()
    return losses, abs(float(t.detach()) - truth)


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import focus_f64 as F
    import gen_focus_grad as gen
    from conftest import load_state
    ref = gen.gg.build_lens("rf50mm")
    ps = load_state("rf50mm")["pixel_size"]
    pts, _, _ = problem(ref.d_sensor, ref.entrance_pupil()[1])
    G = np.zeros((len(POINTS), KS, KS), np.float32)
    gen.gg.set_seed(0)
    with gen.dg.Draws(replay=[u.numpy() for u in uniforms()]):
        run = gen.run(ref, pts.numpy(), DP[3], "l", True, G, True, ks=KS, spp=SPP, dp=DP[:3], seed=0)
    s0 = run["s0"]
    rays, chief = ([torch.from_numpy(a) for a in b] for b in (run["rays"], run["chief"]))
    with torch.no_grad():
        tL, tR = F.psf_lr(rays, chief, torch.tensor(s0 + OFFSET, dtype=torch.float64), s0, ps, KS, DP, mask_dtype=torch.float64)

    def psfs(t):
        L, R = F.psf_lr(rays, chief, t, s0, ps, KS, DP, mask_dtype=torch.float64)
        return ((L - tL) ** 2).sum() + ((R - tR) ** 2).sum()
    losses, dist = adam(psfs, s0, s0 + OFFSET)
    print("losses", " ".join(f"{v:.4e}" for v in losses))
    print(f"loss ratio last / first = {losses[-1] / losses[0]:.4f}   |t - truth| / offset = {dist / OFFSET:.4f}")


if __name__ == "__main__":
    main()
