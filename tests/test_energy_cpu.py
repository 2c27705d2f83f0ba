"""The energy of a dual-pixel PSF without a GPU: the float64 restatement (tests/energy_f64.py) against the raw grid sums
of tests/splat_f64.py where no ray is cut, its autograd against central differences, render_psf.photometric_scale
against a hand-written formula, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest
import torch

from energy_f64 import energy_f64, energy_grad_f64
from splat_f64 import boundaries, fragile_x, splat_f64, sub_pixel_areas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rays(rng, S, N, ks, ps, inside=0.9, dead=0.15):
    """Synthetic sensor-plane rays, positions within `inside` of the half window around centres of 0."""
    half = (ks / 2 - 0.5) * ps
    o = rng.uniform(-inside * half, inside * half, (S, N, 2)).astype(np.float32)
    d = rng.normal(0, 0.2, (S, N, 3))
    d[..., 2] = 1.0
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    ra = (rng.random((S, N)) >= dead).astype(np.float32)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return f(o[..., 0]), f(o[..., 1]), f(d[..., 0]), f(d[..., 2]), f(ra)


@pytest.mark.parametrize("r", [0.35, 0.5, 0.62, 0.8])
def test_energy_equals_the_raw_grid_sums_when_no_ray_is_cut(r):
    """The four bilinear taps of a ray sum to 1, so with every live ray inside the window the raw grids of splat_f64
    sum to the energy: the new quantity is tied to the restatement that is already held against the reference."""
    ks, ps, S, N = 21, 0.00431, 700, 4
    ox, oy, dx, dz, ra = _rays(np.random.default_rng(int(r * 100)), S, N, ks, ps)
    h, f, w = 0.78, 1.44, 0.3
    E = energy_f64(dx, dz, ra, h, f, w, r)
    L, R = splat_f64(ox, oy, dx, dz, ra, torch.zeros((N, 2), dtype=torch.float64), ps, ks, h, f, w, r)
    sums = torch.stack((L.sum((1, 2)), R.sum((1, 2))), -1)
    rel = float(((E[:, :2] - sums).abs() / sums.abs()).max())
    print(f"r {r}: |energy - raw grid sums| / sums = {rel:.2e}")
    assert bool((sums > 0).all()) and rel <= 1e-12
    assert torch.equal(E[:, 2], ra.double().sum(0))
    # and the cut rays are what tells them apart: point 0's rays moved out of the window leave its grids empty, while
    # the energy, which reads no position, stays
    ox2 = ox.clone()
    ox2[:, 0] = 2 * (ks / 2) * ps
    L2, R2 = splat_f64(ox2, oy, dx, dz, ra, torch.zeros((N, 2), dtype=torch.float64), ps, ks, h, f, w, r)
    assert float(L2[0].sum()) == 0 == float(R2[0].sum()) and float(E[0, :2].min()) > 0
    assert torch.equal(L2[1:], L[1:])


@pytest.mark.parametrize("r", [0.35, 0.5, 0.62, 0.8])
def test_restatement_autograd_matches_central_differences(r):
    """h, f, w and t by float64 central differences, on rays no boundary of which lies within 1e-3 of a clamp edge: those
    at which the derivative jumps (fragile_x), |x| = r, where the chord has a square-root singularity, and the u clamp
    |x| = sqrt(r^2 - 1/4) of the big-r model, where it has a kink -- a step of 2e-5 then crosses none, and the central
    difference is as good as its step allows."""
    rng = np.random.default_rng(int(r * 1000))
    S, N = 400, 3
    _, _, dx, dz, ra = _rays(rng, S, N, 21, 0.00431)
    h, f, w = 0.71, 1.52, 0.33
    t = -dx.double() / dz.double()
    keep = ~fragile_x(t, h, f, w, r, band=1e-3)
    x = torch.cat(boundaries(t, h, f, w)).abs()
    for edge in ([r] if r <= 0.5 else [float(np.sqrt(r * r - 0.25))]):
        keep &= ~((x - edge).abs() < 1e-3).any(0)
    ra = ra * keep
    assert int((ra != 0).sum()) > 0.5 * S * N
    G = torch.randn((N, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    got = energy_grad_f64(dx, dz, ra, h, f, w, r, G)

    def loss(hh, ff, ww, tt):
        sl, sr = sub_pixel_areas(tt, hh, ff, ww, r)
        return float(((ra.double() * sl).sum(0) * G[:, 0] + (ra.double() * sr).sum(0) * G[:, 1]).sum())
    # central differences at two steps, extrapolated (4 D(s / 2) - D(s)) / 3: the s^2 term is gone, and the rounding of
    # the loss, some 1e-13 / s, stays under 1e-8
    step = 2e-5

    def extrapolated(diff):
        return (4 * diff(step / 2) - diff(step)) / 3

    def by_parameter(k, s):
        hi, lo = [h, f, w], [h, f, w]
        hi[k] += s
        lo[k] -= s
        return (loss(*hi, t) - loss(*lo, t)) / (2 * s)
    for k, name in enumerate("hfw"):
        fd = extrapolated(lambda s: by_parameter(k, s))
        rel = abs(fd - float(got["theta"][k])) / abs(fd)
        print(f"r {r} d/d{name}: autograd {float(got['theta'][k]):.9e} central difference {fd:.9e} (relative {rel:.1e})")
        assert abs(fd) > 0 and rel <= 1e-7
    # t: every ray's own derivative, dLoss/dt = -g_dx * dz (t = -dx / dz)
    dt = -got["g_dx"] * dz.double()
    def by_t(s):
        sl_hi, sr_hi = sub_pixel_areas(t + s, h, f, w, r)
        sl_lo, sr_lo = sub_pixel_areas(t - s, h, f, w, r)
        return ra.double() * ((sl_hi - sl_lo) * G[:, 0] + (sr_hi - sr_lo) * G[:, 1]) / (2 * s)
    fd = extrapolated(by_t)
    rel = float((fd - dt).abs().max() / dt.abs().max())
    print(f"r {r} d/dt per ray: worst |autograd - central difference| / max|term| = {rel:.1e}")
    assert float(dt.abs().max()) > 0 and rel <= 1e-7
    # and dz's share is the same derivative through t = -dx / dz: g_dz = dLoss/dt * dx / dz^2
    want_dz = dt * dx.double() / dz.double() ** 2
    assert float((got["g_dz"] - want_dz).abs().max()) <= 1e-12 * float(want_dz.abs().max())
    dead = ra == 0
    assert bool((got["g_dx"][dead] == 0).all()) and bool((got["g_dz"][dead] == 0).all())


def test_photometric_scale_values_and_autograd_match_the_hand_written_formula():
    from sdirt_amd.render_psf import photometric_scale
    g = torch.Generator().manual_seed(5)
    Dz, Gy, Gx, ks = 2, 3, 4, 5
    psf = torch.rand((Dz, Gy, Gx, 2, ks, ks), dtype=torch.float64, generator=g)
    psf = psf / psf.sum((-1, -2), keepdim=True)
    E = torch.rand((Dz, Gy, Gx, 3), dtype=torch.float64, generator=g) + 0.2
    W = torch.randn(psf.shape, dtype=torch.float64, generator=g)
    p1, e1 = psf.clone().requires_grad_(), E.clone().requires_grad_()
    out = photometric_scale(p1, e1)
    (W * out).sum().backward()
    # by hand: gain[n, s] = E[n, s] / m, m = sum(E[:, :2]) / (2 n_nodes)
    n = Dz * Gy * Gx
    m = float(E[..., :2].sum()) / (2 * n)
    want = psf * (E[..., :2] / m)[..., None, None]
    assert float((out.detach() - want).abs().max()) <= 1e-15
    sums = out.detach().sum((-1, -2))
    assert abs(float(sums.mean()) - 1.0) <= 1e-14                       # the mean of the L/R kernel sums is 1
    assert float((sums - E[..., :2] / m).abs().max()) <= 1e-14
    # d/dpsf = W gain; d/dE[n, s] = a[n, s] / m - sum(a E) / (2 n m^2), a[n, s] = sum_pixels W psf; column 2: nothing
    a = (W * psf).sum((-1, -2))
    want_e = a / m - (a * E[..., :2]).sum() / (2 * n * m * m)
    assert float((p1.grad - W * (E[..., :2] / m)[..., None, None]).abs().max()) <= 1e-13
    assert float((e1.grad[..., :2] - want_e).abs().max()) <= 1e-12 * float(want_e.abs().max())
    assert bool((e1.grad[..., 2] == 0).all())
    # equal energies: the volume as it was
    same = photometric_scale(psf, torch.full((Dz, Gy, Gx, 3), 0.37, dtype=torch.float64))
    assert float((same - psf).abs().max()) <= 1e-15
    # a chromatic volume: wavelength by wavelength, each by its own mean
    psf3 = torch.stack((psf, psf.flip(0), psf.flip(1)))
    E3 = torch.stack((E, 3.0 * E.flip(0), 0.1 * E.flip(1)))
    out3 = photometric_scale(psf3, E3)
    for c in range(3):
        assert float((out3[c] - photometric_scale(psf3[c], E3[c])).abs().max()) <= 1e-15
    # fp32 PSFs stay fp32 and the shapes must agree
    assert photometric_scale(psf.float(), E).dtype == torch.float32
    with pytest.raises(ValueError):
        photometric_scale(psf, E[0])
    with pytest.raises(ValueError):
        photometric_scale(psf, E[..., :2])


def test_volume_has_a_trailing_energy_field_and_the_abi_declares_the_entries():
    import dataclasses
    from sdirt_amd import _lib
    from sdirt_amd.render_psf import PSFVolume
    import inspect
    assert list(inspect.signature(PSFVolume).parameters) == ["psf", "x_nodes", "y_nodes", "z_nodes", "d_min", "d_max", "wvln",
                                                               "energy"]
    z, E = torch.zeros(1), torch.ones((1, 1, 1, 3), dtype=torch.float64)
    assert PSFVolume(None, z, z, z, -200.0, -20000.0).energy is None
    v = PSFVolume(None, z, z, z, -200.0, -20000.0, (0.589,), E)
    assert v.energy is E and dataclasses.replace(v, d_min=-100.0).energy is E
    assert PSFVolume(None, z, z, z, -200.0, -20000.0, energy=E).energy is E
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdirt_dp.h")).read(), flags=re.S)
    h = _lib.lib()
    for name in ("sdirt_dp_energy", "sdirt_dp_energy_grad"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert len(_lib.SIGNATURES["sdirt_dp_energy"][1]) == 8 and len(_lib.SIGNATURES["sdirt_dp_energy_grad"][1]) == 11
    assert h.sdirt_abi_version() == 4 == _lib.ABI_VERSION
    assert "#define SDIRT_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()


def test_psf_lr_refuses_energy_with_defer_or_without_dp():
    from conftest import make_lens
    lens = make_lens("rf50mm", "cpu")
    pts = torch.tensor([[0.0, 0.0, -1500.0]])
    for kw in (dict(defer=True), dict(_default_r_zero=True), dict(dp=None)):
        with pytest.raises(ValueError):
            lens.psf_lr(pts, ks=21, spp=64, energy=True, **kw)
