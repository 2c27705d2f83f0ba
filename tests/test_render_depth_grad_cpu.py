"""The layered render's backward into the layer depths and texel scales, the parts that need no GPU,
on synthetic rays: px_l = ox + sx (z_l - oz), py_l alike, built in float64 here and rounded to fp32 landings; a fifth of
the rays dead, every other of those on NaN, +-inf, +-3e38; binary and fractional coverage; up to 16 layers; 1-texel
extents.

  1. the product's torch restatement (layer_depth_grads_float64) against the independent one
     (tests/render_depth_grad_f64.py) within 2 (n + rho) 2^-53 sum|term|, rho = 5 L + 33 counted in §7s;
  2. ... against torch.autograd through layer_sums_float64 with the landings as differentiable leaves;
  3. ... against a central difference of the numpy FORWARD restatement (tests/render_layers_f64.py) in z_l and in
     inv_texel_l, with a bound derived here from the step's third-order term and the fp32 spacing of u, v;
  4. a linear-ramp texture under a null alpha: gz = sum q (-inv sx) slope, rays outside the texture exactly 0;
  5. every new argument error; the entry in the header, the binding and the library."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_lens
import render_depth_grad_f64 as RZ
import render_layers_f64 as RL
from render_rt_f64 import F32, tap_origin
from test_render_layers_cpu import H, W, record

ENTRY = "sdirt_render_layers_depth_grad"
U = 2.0 ** -53
OZ = 5.0                                                        # where the trace leaves the rays


def scene(L, Ht, Wt, S, seed, shared=False, frac=True, band=0.0):
    """Synthetic rays and a scene: -> dict.  The rays' slopes are those of the fp32 directions (dx / dz in float64, as
    §7s takes them); `land(zs)` gives the fp32 landings on layers at depths zs.  band > 0: rays whose fu or fv lies
    within `band` of a texel boundary on any layer are drawn again until none is left (asserted)."""
    rng = np.random.default_rng(seed)
    inv = [0.37 * (1 + Wt) ** 0.5 * (1 + 0.21 * l) for l in range(L)]
    zs = [-400.0 - 90.0 * l for l in range(L)]
    span = 90.0 * max(L - 1, 1)
    ex, ey = (Wt / 2) / inv[0], (Ht / 2) / inv[0]
    shape = (S, H, W)

    def draw():
        dz = -rng.uniform(0.9, 1.0, shape)
        sx = rng.choice([-1.0, 1.0], shape) * rng.uniform(0.1, 1.0, shape) * 0.5 * ex / span
        sy = rng.choice([-1.0, 1.0], shape) * rng.uniform(0.1, 1.0, shape) * 0.5 * ey / span
        dirs = np.stack((sx * dz, sy * dz, dz)).astype(F32)
        x0 = rng.uniform(-1.5, 1.5, shape) * ex                 # the landing on layer 0 reaches 1.5 x the half extent
        y0 = rng.uniform(-1.5, 1.5, shape) * ey
        return dirs, x0, y0

    dirs, x0, y0 = draw()

    def slopes_of(d):
        return d[0].astype(np.float64) / d[2].astype(np.float64), d[1].astype(np.float64) / d[2].astype(np.float64)

    def land_of(d, x0, y0, depths):
        sx, sy = slopes_of(d)
        ox, oy = x0 - sx * (zs[0] - OZ), y0 - sy * (zs[0] - OZ)
        px = np.stack([ox + sx * (z - OZ) for z in depths]).astype(F32)
        py = np.stack([oy + sy * (z - OZ) for z in depths]).astype(F32)
        return px, py

    def flagged(d, x0, y0):
        px, py = land_of(d, x0, y0, zs)
        bad = np.zeros(shape, bool)
        for l in range(L):
            _, _, fu, fv = tap_origin(px[l], py[l], inv[l], Ht, Wt)
            bad |= (fu < band) | (fu > 1 - band) | (fv < band) | (fv > 1 - band)
        return bad

    if band > 0:
        for _ in range(200):
            bad = flagged(dirs, x0, y0)
            if not bad.any():
                break
            d2, x2, y2 = draw()
            dirs, x0, y0 = np.where(bad, d2, dirs), np.where(bad, x2, x0), np.where(bad, y2, y0)
        assert not flagged(dirs, x0, y0).any()
    ra = (rng.uniform(size=shape) >= 0.2).astype(F32)
    w = rng.uniform(0.0, 1.0, (2,) + shape).astype(F32)
    specials = [np.nan, np.inf, -np.inf, 3e38, -3e38]
    dead_special = np.flatnonzero(ra == 0)[::2]

    def land(depths):
        px, py = land_of(dirs, x0, y0, depths)
        for n, idx in enumerate(dead_special):
            for l in range(len(depths)):
                px[l].flat[idx] = specials[(n + l) % 5]
                py[l].flat[idx] = specials[(n // 5 + l) % 5]
        return px, py

    dirs_rec = dirs.copy()
    for n, idx in enumerate(dead_special):
        for c in range(3):
            dirs_rec[c].flat[idx] = specials[(n + c) % 5]
    alpha = (rng.uniform(size=(L, Ht, Wt)) < 0.5).astype(F32)
    if frac:
        alpha = np.where(rng.uniform(size=alpha.shape) < 0.5, rng.uniform(size=alpha.shape), alpha).astype(F32)
    tex = rng.uniform(-0.25, 0.75, ((3, Ht, Wt) if shared else (L, 3, Ht, Wt))).astype(F32)
    gnum = rng.standard_normal((2, 3, H, W))
    return dict(L=L, Ht=Ht, Wt=Wt, S=S, inv=inv, zs=zs, dirs=dirs_rec, slopes=slopes_of(dirs), land=land, ra=ra, w=w,
                alpha=alpha, tex=tex, gnum=gnum)


STACKS = [(1, 2, 3, 8, False, False), (2, 5, 141, 5, True, True), (3, 11, 280, 8, False, True), (5, 1, 7, 5, False, False),
          (16, 5, 9, 8, True, True), (2, 1, 1, 5, False, True), (3, 7, 1, 8, True, True)]


# ------------------------------------------------------------------------------------ 1. torch against the restatement
@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("L, Ht, Wt, S, shared, frac", STACKS)
def test_the_product_s_restatement_equals_the_independent_one(L, Ht, Wt, S, shared, frac, views):
    from sdirt_amd.render_rt import layer_depth_grads_float64
    sc = scene(L, Ht, Wt, S, 1300 + 10 * L + Wt, shared, frac)
    px, py = sc["land"](sc["zs"])
    gnum, w = sc["gnum"][:views], sc["w"][:views]
    ref = RZ.depth_grads_f64(px, py, sc["ra"], w, sc["dirs"], sc["alpha"], sc["tex"], sc["inv"], gnum)
    got, mags = layer_depth_grads_float64(record(px, py, sc["ra"], sc["w"]), sc["dirs"], sc["alpha"], sc["tex"], sc["inv"],
                                          gnum, return_abs=True)
    assert got.dtype == torch.float64 and got.shape == (L, 2)
    tol = RZ.bound(ref["n"], L, ref["abs"].T).T
    worst = float((np.abs(got.numpy() - ref["grad"]) / np.where(tol > 0, tol, 1)).max())
    print(f"L {L}, {Ht} x {Wt}, V {views}: worst |torch - restatement| / bound {worst:.3f}, n {ref['n'].tolist()}")
    assert (np.abs(got.numpy() - ref["grad"]) <= tol).all(), worst
    assert (np.abs(mags.numpy() - ref["abs"]) <= tol).all()
    assert np.isfinite(ref["grad"]).all() and ref["n"][0] == (sc["ra"] != 0).sum()
    if Wt > 1:
        assert (ref["grad"][:, 0] != 0).all() and (ref["abs"] > 0).all()
    else:                                                       # a 1-texel extent along x: no derivative in u at all
        assert (ref["Pu"] == 0).all()
    if Ht == 1:
        assert (ref["Pv"] == 0).all()
    # a landing outside the texture along x: both columns are one texel, Pu is exactly 0
    live = sc["ra"] != 0
    outside = live[None] & ((ref["c0"] < 0) | (ref["c0"] >= Wt - 1))
    assert outside.any() and (ref["Pu"][outside] == 0).all()
    # an opaque stack (alpha=None) is alpha == 1 in every bit, and meets layer 0 only
    none = layer_depth_grads_float64(record(px, py, sc["ra"], sc["w"]), sc["dirs"], None, sc["tex"], sc["inv"], gnum)
    ones = layer_depth_grads_float64(record(px, py, sc["ra"], sc["w"]), sc["dirs"], np.ones_like(sc["alpha"]), sc["tex"],
                                     sc["inv"], gnum)
    assert torch.equal(none, ones) and bool((none[1:] == 0).all())
    opaque = RZ.depth_grads_f64(px, py, sc["ra"], w, sc["dirs"], None, sc["tex"], sc["inv"], gnum)
    assert (np.abs(none.numpy() - opaque["grad"]) <= RZ.bound(opaque["n"], L, opaque["abs"].T).T).all()


def test_rho_is_the_count_of_section_7s():
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = txt[txt.index("## 7s."):txt.index("## 8. Out of scope")]
    assert "5 L + 33" in sec and RZ.rho(16) == 113


# ------------------------------------------------------------------------------------ 2. torch against autograd
@pytest.mark.parametrize("L, Ht, Wt, S, shared", [(1, 2, 3, 8, False), (3, 5, 9, 5, True), (16, 2, 3, 8, False)])
def test_the_product_s_restatement_equals_autograd_through_the_landings(L, Ht, Wt, S, shared):
    """The landings are float64 leaves; layer_sums_float64 casts them to fp32 and forms u, v, fu, fv in fp32, so
    autograd's way back to a landing carries at most four fp32 roundings (the cast of fu's adjoint, the product with
    inv, and the fp32 sum of the coverage's and the colour's chains at the landing): (4 2^-24 + 64 n 2^-53) sum|term|.
    The chain to z_l is the slope, the chain to inv_l is px_l / inv_l (u depends on the product px inv alone)."""
    from sdirt_amd.render_rt import layer_depth_grads_float64, layer_sums_float64
    sc = scene(L, Ht, Wt, S, 1500 + L, shared, True)
    px, py = sc["land"](sc["zs"])
    live = sc["ra"] != 0
    rec = record(px, py, sc["ra"], sc["w"])
    leaf = torch.where(torch.from_numpy(live), rec.double(), torch.zeros((), dtype=torch.float64)).requires_grad_()
    num, _, _ = layer_sums_float64(leaf, sc["alpha"], sc["tex"], sc["inv"])
    (torch.from_numpy(sc["gnum"]) * num).sum().backward()
    g = leaf.grad.numpy()
    assert np.isfinite(g).all() and (g[3:, ~live] == 0).all()
    sx, sy = sc["slopes"]
    auto = np.zeros((L, 2))
    for l in range(L):
        gx, gy = g[3 + 2 * l], g[4 + 2 * l]
        inv = float(F32(sc["inv"][l]))
        auto[l, 0] = np.where(live, gx * sx + gy * sy, 0.0).sum()
        x, y = np.where(live, px[l], F32(0)).astype(np.float64), np.where(live, py[l], F32(0)).astype(np.float64)
        auto[l, 1] = np.where(live, (gx * x + gy * y) / inv, 0.0).sum()
    got, mags = layer_depth_grads_float64(rec, sc["dirs"], sc["alpha"], sc["tex"], sc["inv"], sc["gnum"], return_abs=True)
    tol = (4 * 2.0 ** -24 + 64 * live.size * U) * mags.numpy()
    worst = float((np.abs(auto - got.numpy()) / tol).max())
    print(f"L {L}: grad {got.numpy()[0].tolist()}, worst |autograd - restatement| / tolerance {worst:.3f}")
    assert (np.abs(auto - got.numpy()) <= tol).all(), worst
    assert bool((got.abs() > 0).all())


# ------------------------------------------------------------------------------------ 3. central difference of the forward
@pytest.mark.parametrize("L, Ht, Wt, S", [(1, 5, 9, 8), (3, 5, 9, 8), (3, 11, 40, 5)])
def test_the_gradient_is_the_central_difference_of_the_numpy_forward(L, Ht, Wt, S):
    """F = <gnum, num> of the FORWARD restatement, moved in one z_l or one inv_l by +-h.  Rays within BAND of a texel
    boundary were drawn again (none is left: asserted), and h moves no ray's u or v by more than STEP < BAND, so every
    ray stays in its bilinear cell.  There F is a polynomial in the moved quantity x: F = const + sum_rays T_l (a_l (D_l -
    R_{l+1})), a_l and D_l bilinear in (u, v), u and v linear in x, so a''' = D''' = 0 and
      F''' = sum_rays T_l (3 a'' D' + 3 a' D''),    a' = a_u u' + a_v v',    a'' = 2 a_uv u' v'   (D alike).
    Bound on |central difference - gradient|:
      h^2 / 6 sum_rays 3 T_l (|a''| |D'| + |a'| |D''|) with every factor's magnitude            (the third-order term; the
                                                                                                 fifth-order one is 0)
      + (4 * 2^-24 * Umax / h') sum_rays (|Pu| + |Pv|)                                            (the fp32 spacing)
    The second: the forward forms u from an fp32 landing (half a spacing of px times inv), one product, one
    difference and u - 0.5, each rounded to fp32: at most 4 half-spacings of the largest |u| or |v| a ray reaches,
    Umax = the power of two above 1.25 max(Wt, Ht) + 1; a change du of a ray's u changes F by at most |Pu| du (F is
    continuous and piecewise polynomial in u); both ends of the difference carry it, over 2 h: per unit of u' h = h'.
    Written as sum|term| it is (4 * 2^-24 * Umax) (|Pu| |u'| + |Pv| |v'|) / (|u'| h) <= that / h' with h' the smallest
    step a ray takes -- so the test uses the per-ray form sum (|Pu| + |Pv|) 4 2^-24 Umax / h."""
    from sdirt_amd.render_rt import layer_depth_grads_float64
    BAND, STEP = 0.05, 0.02
    sc = scene(L, Ht, Wt, S, 1700 + L + Wt, False, True, band=BAND)
    zs, inv, gnum, live = sc["zs"], sc["inv"], sc["gnum"], sc["ra"] != 0
    inv = [float(F32(v)) for v in inv]
    px, py = sc["land"](zs)
    got = layer_depth_grads_float64(record(px, py, sc["ra"], sc["w"]), sc["dirs"], sc["alpha"], sc["tex"], inv, gnum).numpy()
    ref = RZ.depth_grads_f64(px, py, sc["ra"], sc["w"], sc["dirs"], sc["alpha"], sc["tex"], inv, gnum)
    sx, sy = sc["slopes"]
    Umax = 2.0 ** np.ceil(np.log2(1.25 * max(Wt, Ht) + 1))

    def F(depths, invs):
        x, y = sc["land"](depths)
        num = RL.layer_sums_f64(x, y, sc["ra"], sc["w"], sc["alpha"], sc["tex"], invs)[0]
        return float((gnum * num).sum())

    base = RZ.RG.layer_grads_f64(px, py, sc["ra"], sc["w"], sc["alpha"], sc["tex"], inv, gnum)
    wr = np.where(live, sc["w"].astype(np.float64) * sc["ra"].astype(np.float64), 0.0)
    qa = wr[0] * np.abs(gnum[0])[:, None] + wr[1] * np.abs(gnum[1])[:, None]
    for l in range(L):
        x = np.where(live, px[l], F32(0)).astype(np.float64)
        y = np.where(live, py[l], F32(0)).astype(np.float64)
        idx, _ = RZ.RG.taps(x.astype(F32), y.astype(F32), inv[l], Ht, Wt)
        _, _, fu, fv = tap_origin(x.astype(F32), y.astype(F32), inv[l], Ht, Wt)
        fu, fv = fu.astype(np.float64), fv.astype(np.float64)

        def mixed(planes):                                      # |v11 - v10 - v01 + v00|
            p = planes.astype(np.float64).reshape(planes.shape[0], -1)
            return np.abs(p[:, idx[3]] - p[:, idx[2]] - p[:, idx[1]] + p[:, idx[0]])

        aua, ava = (v[0] for v in RZ.slopes(sc["alpha"][l:l + 1], idx, fu, fv, magnitudes=True))
        tua, tva = RZ.slopes(sc["tex"][l], idx, fu, fv, magnitudes=True)
        a_uv, D_uv = mixed(sc["alpha"][l:l + 1])[0], (qa * mixed(sc["tex"][l])).sum(0)
        Du, Dv = (qa * tua).sum(0), (qa * tva).sum(0)
        Tl = base["T_before"][l]
        for comp, (du, dv) in enumerate([(inv[l] * np.abs(sx), inv[l] * np.abs(sy)), (np.abs(x), np.abs(y))]):
            h = STEP / max(float(du[live].max()), float(dv[live].max()))
            assert h * max(float(du[live].max()), float(dv[live].max())) + 4 * 2.0 ** -24 * Umax < BAND
            if comp == 0:
                zp, zm = list(zs), list(zs)
                zp[l], zm[l] = zs[l] + h, zs[l] - h
                cd = (F(zp, inv) - F(zm, inv)) / ((zp[l] - zs[l]) + (zs[l] - zm[l]))
            else:
                h = 2.0 ** np.floor(np.log2(h))                  # a power of two far above fp32's spacing at inv: inv +- h
                ip, im = list(inv), list(inv)                   # are fp32 numbers, and the two steps are equal
                ip[l], im[l] = float(F32(inv[l] + h)), float(F32(inv[l] - h))
                assert ip[l] - inv[l] == inv[l] - im[l] == h
                cd = (F(zs, ip) - F(zs, im)) / (2 * h)
            a1, a2 = aua * du + ava * dv, 2 * a_uv * du * dv
            D1, D2 = Du * du + Dv * dv, 2 * D_uv * du * dv
            third = h * h / 6 * np.where(live, 3 * Tl * (a2 * D1 + a1 * D2), 0.0).sum()
            # |Pu| + |Pv| with every factor's magnitude: sum|term| of the restatement with unit chains
            spacing = 4 * 2.0 ** -24 * Umax / h * np.where(live, np.abs(ref["Pu"][l]) + np.abs(ref["Pv"][l]), 0.0).sum()
            f64 = 64 * live.size * U * ref["abs"][l, comp] + 4 * live.size * U * np.abs(gnum).sum() / h
            tol = third + spacing + f64
            err = abs(cd - got[l, comp])
            print(f"L {L} layer {l} {'z' if comp == 0 else 'inv'}: gradient {got[l, comp]:+.6e}, central difference "
                  f"{cd:+.6e}, |difference| {err:.2e}, bound {tol:.2e} = third {third:.2e} + spacing {spacing:.2e}")
            assert err <= tol, (l, comp, err, tol)
            assert abs(got[l, comp]) > 4 * tol                  # the bound is no larger than a quarter of the gradient


# ------------------------------------------------------------------------------------ 4. a ramp under a null alpha
def test_a_linear_ramp_has_the_gradient_of_its_slope_across_texel_boundaries():
    """tex[k, r, c] = s_k c + b_k with powers of two s_k: bilinear interpolation of a ramp is exactly linear inside the
    texture, v01 - v00 = s_k and v10 - v00 = 0 in every cell, so Pu = sum_k q_k s_k, Pv = 0 and the ray's term is
    q . s (-inv sx), whichever cell it lands in.  Outside the texture along x the term is exactly 0."""
    from sdirt_amd.render_rt import layer_depth_grads_float64
    Ht, Wt, S = 4, 12, 8
    sc = scene(1, Ht, Wt, S, 1900, True, False)
    s = np.array([0.25, -0.5, 0.125])
    tex = (s[:, None, None] * np.arange(Wt)[None, None, :] + np.array([0.5, 4.0, -1.0])[:, None, None]
           + np.zeros((3, Ht, Wt))).astype(F32)
    px, py = sc["land"](sc["zs"])
    live = sc["ra"] != 0
    got, mags = layer_depth_grads_float64(record(px, py, sc["ra"], sc["w"]), sc["dirs"], None, tex, sc["inv"], sc["gnum"],
                                          return_abs=True)
    c0, _, _, _ = tap_origin(np.where(live, px[0], F32(0)), np.where(live, py[0], F32(0)), sc["inv"][0], Ht, Wt)
    inside = live & (c0 >= 0) & (c0 < Wt - 1)
    wr = np.where(live, sc["w"].astype(np.float64) * sc["ra"].astype(np.float64), 0.0)
    q = wr[0] * sc["gnum"][0][:, None] + wr[1] * sc["gnum"][1][:, None]
    sx, _ = sc["slopes"]
    Pu = q[0] * s[0] + q[1] * s[1] + q[2] * s[2]
    inv = float(F32(sc["inv"][0]))
    terms = np.where(inside, inv * (0.0 * Pu - Pu * sx), 0.0)
    n = int(inside.sum())
    assert 0.3 * live.sum() < n < 0.9 * live.sum() and len(np.unique(c0[inside])) == Wt - 1     # every cell, and outside
    tol = 2 * (n + 8) * U * np.abs(terms).sum()
    print(f"ramp: gz {float(got[0, 0]):+.9e}, sum q.s (-inv sx) {terms.sum():+.9e}, bound {tol:.2e}")
    assert abs(float(got[0, 0]) - terms.sum()) <= tol
    ref = RZ.depth_grads_f64(px, py, sc["ra"], sc["w"], sc["dirs"], None, tex, sc["inv"], sc["gnum"])
    assert (ref["Pu"][0][live & ~inside] == 0).all() and (ref["Pv"][0] == 0).all()
    assert (ref["Pu"][0][inside] == Pu[inside]).all()            # exact: s_k are powers of two


# ------------------------------------------------------------------------------------ 5. errors, entry
def test_header_declares_the_entry_and_the_library_exports_it():
    import ctypes as C
    from sdirt_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, code)
    assert "#define SDIRT_ABI_VERSION 4" in txt and "DESIGN.md §7s" in txt
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    n_args = len(re.search(r"int\s+%s\s*\((.*?)\);" % ENTRY, code, re.S).group(1).split(","))
    assert restype is C.c_int and len(argtypes) == n_args == 26
    h = _lib.lib()
    assert hasattr(h, ENTRY) and _lib.ABI_VERSION == 4 and h.sdirt_abi_version() == 4
    assert h.sdirt_render_layers_depth_grad(None, None, 0, None, None, 0.0, None, None, 0.0, 1, 1, 1, None, 1, None, None,
                                            None, None, 0, 1, 1, 1, None, None, None, None) != 0
    assert b"null lens" in h.sdirt_last_error()


def test_the_new_arguments_are_refused_before_anything_touches_the_gpu():
    from sdirt_amd import _lib
    from sdirt_amd.render_rt import layer_depth_grad_batch, layer_depth_grads_float64
    lens = make_lens("rf50mm", "cpu")
    lens.prepare_sensor(sensor_res=(4, 6), sensor_size=(1.0, 1.5))
    K = len(lens.surfaces)
    img, alpha = torch.zeros(2, 3, 4, 6), torch.ones(2, 4, 6)
    zs = torch.tensor([-500.0, -1000.0], requires_grad=True)
    sc = torch.tensor([5.0, 10.0], requires_grad=True)
    pts = (torch.zeros(2, 4, 6), torch.zeros(2, 4, 6))
    kw = dict(spp=2, pupil_points=pts)
    # depth_grad=True with return_sums=True, whatever is a tensor
    with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
        lens.render_layers(img, alpha, zs, scales=sc, depth_grad=True, return_sums=True, **kw)
    with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
        lens.render_layers(img, alpha, [-500.0, -1000.0], scales=[5.0, 10.0], depth_grad=True, return_sums=True, **kw)
    with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
        lens.render_plane(img, torch.tensor(-500.0, requires_grad=True), scale=5.0, depth_grad=True, return_sums=True, **kw)
    # the shapes of the tensors that take a gradient
    with pytest.raises(ValueError, match="must be 1-D tensors of 2"):
        lens.render_layers(img, alpha, zs.detach().reshape(2, 1).requires_grad_(), scales=[5.0, 10.0], depth_grad=True, **kw)
    with pytest.raises(ValueError, match="must be 0-d tensors"):
        lens.render_plane(img, torch.tensor([-500.0], requires_grad=True), scale=5.0, depth_grad=True, **kw)
    with pytest.raises(ValueError, match="strictly descending"):
        lens.render_layers(img, alpha, zs.detach().flip(0).requires_grad_(), scales=sc, depth_grad=True, **kw)
    with pytest.raises(ValueError, match="1 scales for 2 depths"):
        lens.render_layers(img, alpha, zs, scales=sc[:1], depth_grad=True, **kw)
    # what is accepted gets as far as asking for the GPU: with and without depth_grad, tensors or not
    for call in (lambda: lens.render_layers(img, alpha, zs, scales=sc, depth_grad=True, **kw),
                 lambda: lens.render_layers(img, alpha, zs, scales=sc, **kw),
                 lambda: lens.render_layers(img, alpha, zs, scales=sc, return_sums=True, **kw),
                 lambda: lens.render_plane(img, torch.tensor(-500.0, requires_grad=True),
                                           scale=torch.tensor(5.0, requires_grad=True), depth_grad=True, **kw),
                 lambda: lens.render_rgbd(img, torch.full((2, 1, 4, 6), -1000.0), layer_depths=zs, scales=sc,
                                          depth_grad=True, **kw)):
        with pytest.raises(_lib.SdirtError, match="GPU only"):
            call()
    # layer_depth_grad_batch
    trips, gnum = [1] * K, torch.zeros(1, 3, 4, 6, dtype=torch.float64)
    depths, inv = [-500.0, -1000.0], [1.0, 2.0]
    with pytest.raises(ValueError, match="2 layers need 2 depths and 2 scales"):
        layer_depth_grad_batch(lens, alpha, img, depths, [1.0], *pts, trips, gnum)
    with pytest.raises(ValueError, match="strictly descending"):
        layer_depth_grad_batch(lens, alpha, img, depths[::-1], inv, *pts, trips, gnum)
    with pytest.raises(ValueError, match="pupil points must be"):
        layer_depth_grad_batch(lens, alpha, img, depths, inv, pts[0], pts[1][:1], trips, gnum)
    with pytest.raises(ValueError, match="trip counts for a lens of"):
        layer_depth_grad_batch(lens, alpha, img, depths, inv, *pts, trips[:-1], gnum)
    for bad in (gnum.float(), gnum[:, :2], torch.zeros(2, 3, 4, 6, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="gnum must be float64"):
            layer_depth_grad_batch(lens, alpha, img, depths, inv, *pts, trips, bad)
    with pytest.raises(ValueError, match="gnum must be float64"):
        layer_depth_grad_batch(lens, alpha, img, depths, inv, *pts, trips, gnum, dp=(0.78, 1.44, 0.3, 0.5))     # V = 2
    with pytest.raises(ValueError, match="layers differ"):
        layer_depth_grad_batch(lens, None, img, depths, [1.0], *pts, trips, gnum)
    with pytest.raises(ValueError, match="float32"):
        layer_depth_grad_batch(lens, None, img.double(), depths, inv, *pts, trips, gnum)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_depth_grad_batch(lens, alpha, img, depths, inv, *pts, trips, gnum)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_depth_grad_batch(lens, None, img[0], depths[:1], [1.0], *pts, trips, gnum, ray_dir=True)
    # layer_depth_grads_float64
    land, rd = torch.zeros(3 + 2 * 2, 2, 4, 6), torch.zeros(3, 2, 4, 6)
    with pytest.raises(ValueError, match="landing record of 7 rows"):
        layer_depth_grads_float64(land[:5], rd, alpha, img, inv, gnum)
    with pytest.raises(ValueError, match="alpha has 2 layers"):
        layer_depth_grads_float64(land[:5], rd, alpha, img[0], [1.0], gnum)
    with pytest.raises(ValueError, match="ray_dir must be"):
        layer_depth_grads_float64(land, rd[:2], alpha, img, inv, gnum)
    with pytest.raises(ValueError, match="gnum must be"):
        layer_depth_grads_float64(land, rd, alpha, img, inv, gnum[:, :2])
    with pytest.raises(ValueError, match="gnum must be"):
        layer_depth_grads_float64(land, rd, alpha, img, inv, torch.zeros(3, 3, 4, 6, dtype=torch.float64))
