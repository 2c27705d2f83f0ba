"""The glass in the float64 restatement of the trace (tests/trace_f64.py): eta_k = n_k(lambda) / n_k+1(lambda) of every
surface as a float64 torch function of glass [K + 1, 2] (columns n, V of every medium; Lensgroup.glass_parameters), so
that torch's own autograd gives dLoss/d(n, V): the yardstick of sdirt_trace2sensor_grad_eta and of `glass_params=`.

An owned medium (an 'n/V' string) is the reference's Cauchy glass, written out here independently of the package:
n(lambda) = n + (n - 1) / (V c1) (1 / lambda_nm^2 - c2), c1 = 1/486.1^2 - 1/656.3^2, c2 = 1/589.3^2 (basics.py:336-338,
355-362).  Every other medium is a constant.  trace_f64's rows take a tensor eta as they are in the curved branch (also
per-ray leaves [M, 1]); its plane branch compares eta with 1, so a refracting plane with a tensor eta is traced here.
"""
import torch

import trace_f64 as T

C1 = 1 / 486.1 ** 2 - 1 / 656.3 ** 2
C2 = 1 / 589.3 ** 2


def eta(glass, lens, wvln):
    """eta [K] float64 at `wvln` [um], differentiable in glass [K + 1, 2]; constants from the lens's Material objects."""
    wv = wvln if wvln < 10 else wvln * 1e-3
    own = lens.glass_owned()
    const = torch.tensor([float(s.mat1.ior(wv)) for s in lens.surfaces] + [float(lens.surfaces[-1].mat2.ior(wv))], dtype=torch.float64)
    n, V = glass[:, 0].double(), glass[:, 1].double()
    V = torch.where(own, V, torch.ones_like(V))
    ior = torch.where(own, n + (n - 1) / (V * C1) * (1 / (wv * 1e3) ** 2 - C2), const)
    return ior[:-1] / ior[1:]


def glass_table(lens, wvln, etas):
    """trace_f64.lens_table(lens, wvln) with eta of row k replaced by etas[k] (a 0-d tensor or per-ray leaves [M, 1]);
    a non-refracting plane (the stop) keeps its float 1."""
    return [(kind, deg, r, (e if (kind != T.PLANE or float(s.mat1.ior(wvln)) != float(s.mat2.ior(wvln))) else 1.0), c0, k0)
            for (kind, deg, r, _, c0, k0), e, s in zip(T.lens_table(lens, wvln), etas, lens.surfaces)]


def _plane(o, d, D, e):
    t = (D - o[:, 2]) / d[:, 2]
    o = o + t.unsqueeze(-1) * d
    n = torch.zeros_like(o)
    n[:, 2] = 1.0
    return o, T._refract(d, n, e)


def trace_f64(o, d, theta, table, trips, d_sensor, checkpoints=None):
    """trace_f64.trace_f64 for a glass_table: the same walk, a refracting plane with a tensor eta traced by _plane."""
    for k, (kind, deg, r_ap, e, c0, k0) in enumerate(table):
        if checkpoints is not None:
            ck = checkpoints[k].double()
            o, d = T._at(ck[:3].t(), o), T._at(ck[3:].t(), d)
        row = theta[:, k].t() if theta.dim() == 3 else theta[k]
        if kind == T.PLANE and torch.is_tensor(e):
            o, d = _plane(o, d, row[0], e)
        else:
            o, d = T.surface_f64(o, d, row, kind, deg, r_ap, e, c0, k0, trips[k])
    if checkpoints is not None:
        ck = checkpoints[len(table)].double()
        o, d = T._at(ck[:3].t(), o), T._at(ck[3:].t(), d)
    t = (d_sensor - o[:, 2]) / d[:, 2]
    return o + t.unsqueeze(-1) * d, d


COVER_GLASS = "1.5168/64.17"


def cover_glass_lens(tmp_path, device):
    """rf50mm with a 1 mm cover glass -- two planes of semi-aperture r_last -- half way between the last surface and the
    sensor, with rf50mm's pinned state: no shipped lens has a refracting plane."""
    import json
    import os

    from conftest import DATA, load_state
    from sdirt_amd import Lensgroup
    data = json.load(open(os.path.join(DATA, "rf50mm.json")))
    st = load_state("rf50mm")
    z0 = (float(data["surfaces"][-1]["z"]) + float(st["d_sensor"])) / 2
    for z, before, after in ((z0, "air", COVER_GLASS), (z0 + 1.0, COVER_GLASS, "air")):
        data["surfaces"].append({"kind": "plane", "semi_aperture": float(data["r_last"]), "z": z, "curvature": 0.0,
                                 "glass_before": before, "glass_after": after})
    path = os.path.join(str(tmp_path), "rf50mm_cover.json")
    with open(path, "w") as f:
        json.dump(data, f)
    lens = Lensgroup(path, sensor_res=(512, 768), post_computation=False, device=device)
    return lens.set_state(d_sensor=st["d_sensor"], hfov=st["hfov"], pupil=(st["pupil_z"], st["pupil_r"]),
                          exit_pupil=(st["exit_pupil_z"], st["exit_pupil_r"]))
