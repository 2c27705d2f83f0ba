"""k_render_layers_dp_grad (csrc/sdirt_render_rt.hip) on the GPU: the layered render's backward into the
dual-pixel parameters h, f, w -- the forward's rays again, the weights' derivative per ray, one row of three float64
sums per workgroup.

  1. the kernel against tests/render_dp_grad_f64.py (written from the text of §7r) on the forward's own landing record
     and the kernel's recorded x_tan, within 1e-5 sum|term| per component (the bar tests/test_gpu_energy.py holds for
     the same derivative code on the same fp32 decisions);
  2. the recorded x_tan ties to the forward's weight rows;
  3. all 16 instantiations;
  4. plane groups: 5 and 9 planes, gden counted once;
  5. L = 1 with a null alpha, alpha == 1, and render_plane(dp_grad=True), bit for bit;
  6. the same bits: two runs, a side stream, partial overwritten, guard bands;
  7. the autograd surface of render_layers, render_rgbd and render_plane;
  8. kernel against kernel: a central difference through the forward kernel on the occlusion scene;
  9. the entry's refusals.

No atomics: what the kernel adds up IS asserted bit-equal from run to run.  A float64 reference cannot judge a ray within
rounding of a clamp edge at which the derivative jumps (splat_f64.fragile_x): such rays are moved off the edge before
the launch, by a fixed step of their pupil point, and the kernel's own x_tan is checked afterwards.  Sensors, textures
and the seeded alpha stacks are those of test_gpu_render_layers.py and test_gpu_render_raytraced_edges.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_dp_grad_f64 as RD
from splat_f64 import fragile_x, gate_states, sub_pixel_areas
from test_gpu_dp_grad import FRAGILE_CAP
from test_gpu_render_layers import (CASES_3, DEPTHS3, alpha_stack, land_points, layer_inv_texels, lens, rays,  # noqa: F401
                                    stack_depths, staged_layers)
from test_gpu_render_layers_grad import TINY, assert_fp32_of, hand_grads, seeded_gnum
from test_gpu_render_raytraced import DP, DP_BIG, DEV, SMALL, WIDE, WVLN, pupil_points, sensor
from test_gpu_render_raytraced_edges import RAGGED, _guarded, half_cover_scale, inv_texel_of, magnification, texture

from sdirt_amd import _lib
from sdirt_amd.basics import WAVE_RGB, dptr, stream_ptr
from sdirt_amd.render_rt import (gden_from_image_grad, gnum_from_image_grad, layer_batch, layer_dp_grad_batch,
                                 layers_from_rgbd, sensor_axes)

pytestmark = pytest.mark.gpu
FLOOR = 0.05
BAR = 1e-5                                  # tests/test_gpu_energy.py's, for the same derivative on the same decisions
DP_R03, DP_R07 = (0.78, 1.44, 0.3, 0.3), (0.78, 1.44, 0.3, 0.7)
STEP = 0.01                                 # mm a fragile ray's pupil point is moved by: x_tan moves by about 2e-4
POISON = -7.0


def seeded_gden(H, W, seed):
    return torch.randn(2, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(DEV)


def off_the_edges(r, dp):
    """The bundle's pupil points with the rays that fragile_x flags (band 2e-5, on the staged chain's x_tan) moved by
    STEP along x, once -> x2, y2.  The moved share is within FRAGILE_CAP of the live rays (2 rays below 400)."""
    bad = fragile_x(torch.as_tensor(r["x_tan"]), *dp, band=2e-5).to(DEV)
    live = int((r["ra"] != 0).sum())
    moved = int((bad & (r["ra"] != 0)).sum())
    assert moved <= (FRAGILE_CAP * live if live >= 400 else 2), (moved, live)
    return torch.where(bad, r["x2"] + STEP, r["x2"]).contiguous(), r["y2"]


def reference(land, xt, L, alpha, tex, inv, gnum, gden, dp):
    """The restatement of §7r on a launch's landing record and the kernel's recorded x_tan."""
    lx, ly = land_points(land, L)
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return RD.dp_grads_f64(cpu(lx), cpu(ly), cpu(land[0]), cpu(xt), cpu(alpha), cpu(tex), inv, cpu(gnum), cpu(gden), *dp)


def assert_no_fragile(xt, ra, dp):
    bad = fragile_x(xt.cpu(), *dp, band=1e-5) & (ra.cpu() != 0)
    assert not bool(bad.any()), int(bad.sum())


def assert_grad(tag, got, ref):
    """[3] of the kernel against the restatement, per component within BAR sum|term|."""
    got = got.cpu().numpy()
    assert got.shape == (3,) and got.dtype == np.float64
    ratio = np.abs(got - ref["grad"]) / np.maximum(ref["scale"], 1e-300)
    print(f"{tag}: grad {got}, worst |kernel - f64| / sum|term| {ratio.max():.3e} (bar {BAR:.0e}), {ref['n']} rays with a term")
    assert (ratio <= BAR).all(), ratio
    assert (ref["scale"] > 0).all() and np.abs(ref["grad"]).max() > 0


def forward_and_grad(lens, alpha, tex, depths, inv, r, dp, gnum, gden):
    """One forward with a landing record and its dual-pixel backward with the x_tan record, fragile rays moved first."""
    x2, y2 = off_the_edges(r, dp)
    out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, dp, WVLN, landing=True)
    grad, xt = layer_dp_grad_batch(lens, alpha, tex, depths, inv, x2, y2, out["trips"], gnum, gden, dp, WVLN, x_tan=True)
    assert grad.shape == (3,) and grad.dtype == torch.float64 and xt.shape == x2.shape and xt.dtype == torch.float32
    assert_no_fragile(xt, out["landing"][0], dp)
    return out, grad, xt


def assert_gates(tag, xt, ra, dp):
    """g1 and g2 (r > 0.5: u1 too) each open and each closed on at least 1 % of the live rays, counted in float64 on the
    recorded x_tan: a ray counts where the gate of one of its three boundaries is in that state."""
    live = (ra != 0).cpu()
    states = gate_states(xt.cpu()[live], *dp)
    shares = {k: (float(o.any(0).float().mean()), float(c.any(0).float().mean())) for k, (o, c) in states.items()}
    print(f"{tag}: gates (open, closed) " + ", ".join(f"{k} {o:.3f} {c:.3f}" for k, (o, c) in shares.items()))
    for k in ("g1", "g2") + (("u1",) if dp[3] > 0.5 else ()):
        assert min(shares[k]) >= 0.01, (k, shares[k])


# ------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("with_gden", [True, False], ids=["gden", "no-gden"])
@pytest.mark.parametrize("dp", [DP, DP_R03, DP_R07], ids=["r0.5", "r0.3", "r0.7"])
@pytest.mark.parametrize("L, shape, spp, shared, planes, back", CASES_3 + TINY)
def test_gradient_equals_the_float64_restatement(lens, rays, L, shape, spp, shared, planes, back, dp, with_gden):
    Ht, Wt = shape
    depths = stack_depths(L)
    r = rays(spp, depths)
    tag = f"L {L}, {Ht} x {Wt}, spp {spp}, {'shared' if shared else 'per-layer'}, {planes} planes, r {dp[3]}"
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        assert H * W > 256 and (H * W) % 64 != 0                 # several workgroups, a ragged last wave
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, back=back)
        if min(Ht, Wt) == 1:                                     # both taps on one texel: fractional coverage as well
            alpha = alpha * torch.rand(L, Ht, Wt, generator=torch.Generator().manual_seed(5)).to(DEV).clamp_min(0.25)
            alpha[-1] = 1.0
        tex = texture(planes, Ht, Wt, seed=31) if shared else texture(L * planes, Ht, Wt, seed=32).view(L, planes, Ht, Wt)
        gnum = seeded_gnum(2, planes, H, W, seed=33)
        gden = seeded_gden(H, W, seed=34) if with_gden else None
        out, grad, xt = forward_and_grad(lens, alpha, tex, depths, inv, r, dp, gnum, gden)
        ref = reference(out["landing"], xt, L, alpha, tex, inv, gnum, gden, dp)
        assert_gates(tag, xt, out["landing"][0], dp)
        if L > 1 and min(Ht, Wt) > 1:                            # the seeded binary stacks of test_gpu_render_layers.py
            live = out["landing"][0].cpu().numpy() != 0
            early = float((ref["read"][live] < L).mean())
            print(f"{tag}: {early:.3f} of the live rays reach T = 0 before the last layer")
            assert early >= FLOOR, early
        assert_grad(tag, grad, ref)


# ------------------------------------------------------------------------------------ 2. x_tan ties to the forward
@pytest.mark.parametrize("dp", [DP, DP_R03], ids=["r0.5", "r0.3"])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_the_recorded_x_tan_gives_the_forward_s_weight_rows(lens, rays, precision, dp):
    """sub_pixel_areas in float64 at the recorded x_tan against rows 1 and 2 of the forward's landing record, within
    the 4 r^2 3.1e-7 test_gpu_render_layers.py holds the fp32 weights to: (w_L, w_R) = (s_r, s_l)."""
    spp, L, Ht, Wt = 8, 3, 5, 9
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    tol = 4 * dp[3] ** 2 * 3.1e-7
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        alpha, tex = alpha_stack(L, Ht, Wt), texture(2, Ht, Wt, seed=35)
        out, _, xt = forward_and_grad(lens, alpha, tex, depths, inv, r, dp, seeded_gnum(2, 2, H, W, seed=36), None)
        sl, sr = sub_pixel_areas(xt.cpu().double(), *dp)
        w = out["landing"][1:3].cpu().double()
        el, er = float((w[0] - sr).abs().max()), float((w[1] - sl).abs().max())
        print(f"{precision}, r {dp[3]}: max |w_L - s_r| {el:.3e}, max |w_R - s_l| {er:.3e}, bound {tol:.3e}")
        assert float((sr - sl).abs().max()) > 0.1 and el <= tol and er <= tol, (el, er, tol)
        # x_tan is the sampled direction's: every ray has one, dead or live
        assert bool(torch.isfinite(xt).all()) and float(xt.min()) < -0.3 and float(xt.max()) > 0.3


# ------------------------------------------------------------------------------------ 3. every instantiation
@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("dp", [DP, DP_BIG], ids=["small", "big"])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_gradient_of_every_instantiation(lens, rays, precision, dp, planes):
    """k_render_layers_dp_grad<M, DP, NT>: 2 x 2 x 4, at L = 2, each against the landing record of its own forward."""
    spp, Ht, Wt, L = 8, 7, 12, 2
    depths = stack_depths(L)
    r = rays(spp, depths)
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, seed=41)
        tex = texture(L * 4, Ht, Wt, seed=42).view(L, 4, Ht, Wt)[:, :planes].contiguous()
        gnum, gden = seeded_gnum(2, planes, H, W, seed=43), seeded_gden(H, W, seed=44)
        out, grad, xt = forward_and_grad(lens, alpha, tex, depths, inv, r, dp, gnum, gden)
        ref = reference(out["landing"], xt, L, alpha, tex, inv, gnum, gden, dp)
        assert_grad(f"{precision}, r {dp[3]}, {planes} planes", grad, ref)


# ------------------------------------------------------------------------------------ the C entry, directly
def _call_entry(lens, x2, y2, trips, alpha, tex, depths, inv, gnum, gden, partial, xt, dp=DP, stride=None, stream=None):
    H, W = (int(v) for v in lens.sensor_res)
    K, L = len(lens.surfaces), len(depths)
    T, Ht, Wt = (int(v) for v in tex.shape[-3:])
    spp = int(x2.shape[0])
    x1, y1 = sensor_axes(lens, True)
    assert x2.shape == (spp, H, W) and x2.dtype == torch.float32 and x2.is_contiguous() and y2.is_contiguous()
    assert tex.is_contiguous() and L <= _lib.MAX_LAYERS
    assert gnum is None or (gnum.shape == (2, T, H, W) and gnum.dtype == torch.float64 and gnum.is_contiguous())
    assert gden is None or (gden.shape == (2, H, W) and gden.dtype == torch.float64 and gden.is_contiguous())
    assert partial is None or (partial.dtype == torch.float64 and partial.numel() == ((T + 3) // 4) * ((H * W + 255) // 256) * 3)
    assert xt is None or (xt.dtype == torch.float32 and xt.numel() == spp * H * W)
    pupilz, _ = lens.exit_pupil()
    dpp = None if dp is None else C.byref(_lib.DpParams(*(float(v) for v in dp)))
    stride = (T * Ht * Wt if tex.dim() == 4 else 0) if stride is None else stride
    return _lib.lib().sdirt_render_layers_dp_grad(
        lens.dev_lens(WVLN), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
        float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), spp, H, W, dpp, L, (C.c_double * L)(*depths),
        (C.c_double * L)(*inv), dptr(alpha), dptr(tex), stride, T, Ht, Wt, dptr(gnum), dptr(gden), dptr(partial),
        dptr(xt), stream_ptr(lens.device) if stream is None else stream)


# ------------------------------------------------------------------------------------ 4. plane groups
@pytest.mark.parametrize("planes", [5, 9])
def test_plane_groups_are_slices_of_partial_and_gden_counts_once(lens, rays, planes):
    """More than four planes run as further launches: every group of four planes writes a leading slice of `partial`
    of its own -- the restatement on those planes, with gden in the first group only -- and the whole is the
    restatement on all planes with gden once."""
    spp, L, Ht, Wt = 5, 3, 5, 9
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = (int(v) for v in lens.sensor_res)
        rows, groups = (H * W + 255) // 256, (planes + 3) // 4
        assert groups == {5: 2, 9: 3}[planes] and rows == 3
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, seed=45)
        tex = texture(L * planes, Ht, Wt, seed=46).view(L, planes, Ht, Wt)
        gnum, gden = seeded_gnum(2, planes, H, W, seed=47), seeded_gden(H, W, seed=48)
        x2, y2 = off_the_edges(r, DP)
        out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, DP, WVLN, landing=True)
        partial = torch.full((groups, rows, 3), POISON, dtype=torch.float64, device=DEV)
        xt = torch.empty(spp, H, W, dtype=torch.float32, device=DEV)
        assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, gden, partial, xt) == 0
        torch.cuda.synchronize()
        assert_no_fragile(xt, out["landing"][0], DP)
        for g in range(groups):
            sl = slice(4 * g, min(4 * g + 4, planes))
            ref = reference(out["landing"], xt, L, alpha, tex[:, sl], inv, gnum[:, sl], gden if g == 0 else None, DP)
            assert_grad(f"{planes} planes, group {g}", partial[g].sum(0), ref)
        whole = reference(out["landing"], xt, L, alpha, tex, inv, gnum, gden, DP)
        assert_grad(f"{planes} planes, all groups", partial.view(-1, 3).sum(0), whole)
        # gden matters here: without it the sum is another one, by more than the bar
        none = reference(out["landing"], xt, L, alpha, tex, inv, gnum, None, DP)
        assert (np.abs(none["grad"] - whole["grad"]) > 100 * BAR * whole["scale"]).any()
        # ... and the Python call adds the same rows
        grad = layer_dp_grad_batch(lens, alpha, tex, depths, inv, x2, y2, out["trips"], gnum, gden, DP, WVLN)
        assert torch.equal(grad, partial.view(-1, 3).sum(0))


# ------------------------------------------------------------------------------------ 5. reductions
def test_one_opaque_layer_null_alpha_and_render_plane(lens, rays):
    spp, Ht, Wt, planes = 8, 5, 9, 3
    depth = -1000.0
    r = rays(spp, [depth])
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        scale = half_cover_scale(lens, depth, lens.focus_depth)
        inv = [inv_texel_of(lens, scale, Wt)]
        tex = texture(planes, Ht, Wt, seed=61)
        ones = torch.ones(1, Ht, Wt, device=DEV)
        gnum, gden = seeded_gnum(2, planes, H, W, seed=62), seeded_gden(H, W, seed=63)
        out, grad, xt = forward_and_grad(lens, ones, tex, [depth], inv, r, DP, gnum, gden)
        ref = reference(out["landing"], xt, 1, ones, tex, inv, gnum, gden, DP)
        assert_grad("alpha == 1", grad, ref)
        x2, y2 = off_the_edges(r, DP)
        null = layer_dp_grad_batch(lens, None, tex, [depth], inv, x2, y2, out["trips"], gnum, gden, DP, WVLN)
        assert torch.equal(null, grad)                           # c_k = t_{0,k}: bit for bit
        # render_plane(dp_grad=True): img [1, C, Ht, Wt], the loss sum_v <G_v, view_v>, float64 leaves
        leaves = [torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for v in DP[:3]]
        G = torch.randn(2, 1, planes, H, W, generator=torch.Generator().manual_seed(64)).to(DEV)
        kw = dict(spp=spp, wvln=WVLN, scale=scale, pupil_points=(x2, y2))
        vL, vR = lens.render_plane(tex[None], depth, dp=(*leaves, DP[3]), dp_grad=True, **kw)
        plain = lens.render_plane(tex[None], depth, dp=DP, return_sums=True, **kw)
        assert torch.equal(vL, plain[0]) and torch.equal(vR, plain[1]) and vL.grad_fn is not None
        ((vL * G[0]).sum() + (vR * G[1]).sum()).backward()
        num, den = plain[2][:, 0], plain[3]
        gn = gnum_from_image_grad(G[:, 0], den)
        gd = gden_from_image_grad(G[:, 0], num, den)
        hand = layer_dp_grad_batch(lens, None, tex, [depth], inv, x2, y2, out["trips"], gn.contiguous(), gd, DP, WVLN)
        mine = layer_dp_grad_batch(lens, ones, tex, [depth], inv, x2, y2, out["trips"], gn.contiguous(), gd, DP, WVLN)
        got = torch.stack([v.grad for v in leaves])
        print(f"render_plane(dp_grad=True): {got.tolist()}")
        assert got.dtype == torch.float64 and torch.equal(got, hand) and torch.equal(got, mine) and bool((got != 0).all())


def test_a_layer_behind_t0_is_not_read_whatever_it_holds(lens, rays):
    """The forward's walk stops where T reaches 0, and so does this kernel's: behind a fully opaque first layer the
    textures are NaN, and the gradient is the finite one of the first layer alone, bit for bit."""
    spp, L, Ht, Wt, planes = 5, 3, 5, 9, 2
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, seed=66)
        alpha[0] = 1.0
        tex = texture(L * planes, Ht, Wt, seed=67).view(L, planes, Ht, Wt).clone()
        gnum, gden = seeded_gnum(2, planes, H, W, seed=68), seeded_gden(H, W, seed=69)
        _, clean, _ = forward_and_grad(lens, alpha, tex, depths, inv, r, DP, gnum, gden)
        tex[1:] = float("nan")
        out, grad, xt = forward_and_grad(lens, alpha, tex, depths, inv, r, DP, gnum, gden)
        assert bool(torch.isfinite(out["num"]).all()) and bool(torch.isfinite(grad).all()) and torch.equal(grad, clean)
        ref = reference(out["landing"], xt, L, alpha, tex, inv, gnum, gden, DP)
        assert (ref["read"][out["landing"][0].cpu().numpy() != 0] == 1).all()
        assert_grad("NaN behind an opaque layer", grad, ref)


# ------------------------------------------------------------------------------------ 6. the same bits
# 645 pixels: the last workgroup holds 133 live pixels in its waves 0 to 2 and a fourth wave wholly past the sensor
NARROW = dict(res=(5, 129), size=(1.25, 32.25))


@pytest.mark.parametrize("sens, tail", [(RAGGED, 193), (NARROW, 133)], ids=["ragged", "narrow"])
def test_two_runs_and_a_side_stream_give_the_same_bits_inside_guard_bands(lens, rays, sens, tail):
    """The entry directly: partial and x_tan are slices between guard bands; partial, poisoned with -7, is overwritten
    in every element, its rows are ceil(H W / 256) and nothing lies behind them; a second run and a run on a side
    stream give the same bits.  The last workgroup holds live pixels and lanes past the sensor -- on the narrow sensor a
    whole wave of them, which must still hand its zeros to the workgroup's sum."""
    spp, L, Ht, Wt, planes = 5, 3, 5, 141, 3
    depths = list(DEPTHS3)
    with sensor(lens, **sens):
        H, W = (int(v) for v in lens.sensor_res)
        rows = (H * W + 255) // 256
        assert rows == 3 and H * W - 256 * (rows - 1) == tail and (H * W) % 64 != 0
        if sens is RAGGED:
            r = rays(spp, depths)
        else:
            px2, py2 = pupil_points(lens, spp, seed=86)
            _, _, ra, x_tan, _ = staged_layers(lens, px2, py2, depths)
            r = dict(x2=px2, y2=py2, ra=ra, x_tan=x_tan)
        alpha, tex = alpha_stack(L, Ht, Wt), texture(planes, Ht, Wt, seed=83)
        inv = layer_inv_texels(lens, depths, Wt)
        gnum, gden = seeded_gnum(2, planes, H, W, seed=84), seeded_gden(H, W, seed=85)
        x2, y2 = off_the_edges(r, DP)
        out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, DP, WVLN, landing=True)
        runs = []
        for n in range(3):
            partial, p_ok = _guarded(rows * 3, torch.float64)
            xt, x_ok = _guarded(spp * H * W, torch.float32)
            partial.fill_(POISON)
            if n < 2:
                assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, gden, partial, xt) == 0
            else:
                side = torch.cuda.Stream(DEV)
                side.wait_stream(torch.cuda.current_stream(DEV))
                with torch.cuda.stream(side):
                    assert torch.cuda.current_stream(DEV) == side
                    assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, gden, partial, xt,
                                       stream=stream_ptr(lens.device)) == 0
                side.synchronize()
            torch.cuda.synchronize()
            assert p_ok() and x_ok()
            assert not bool((partial == POISON).any()) and bool(torch.isfinite(partial).all())
            assert bool((partial.view(rows, 3)[-1] != 0).all())              # the last workgroup's live pixels count
            runs.append((partial.clone(), xt.clone()))
        for p, x in runs[1:]:
            assert torch.equal(p, runs[0][0]) and torch.equal(x, runs[0][1])
        xt = runs[0][1].view(spp, H, W)
        ref = reference(out["landing"], xt, L, alpha, tex, inv, gnum, gden, DP)
        assert_grad("guarded", runs[0][0].view(rows, 3).sum(0), ref)
        # a null x_tan: the same rows
        partial = torch.full((rows, 3), POISON, dtype=torch.float64, device=DEV)
        assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, gden, partial, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(partial.view(-1), runs[0][0])
        # a row is its workgroup's 256 pixels alone: the adjoints of the last workgroup's pixels zeroed, its row is 0
        gn0, gd0 = gnum.clone(), gden.clone()
        gn0.view(2, planes, -1)[..., 512:] = 0
        gd0.view(2, -1)[..., 512:] = 0
        assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gn0, gd0, partial, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(partial[:2].reshape(-1), runs[0][0][:6]) and not bool(partial[2].any())
        # ... and the last row alone is the restatement on the last workgroup's pixels
        gn1, gd1 = gnum.clone(), gden.clone()
        gn1.view(2, planes, -1)[..., :512] = 0
        gd1.view(2, -1)[..., :512] = 0
        last = reference(out["landing"], xt, L, alpha, tex, inv, gn1, gd1, DP)
        assert_grad(f"the last workgroup's {tail} pixels", runs[0][0].view(rows, 3)[2], last)


# ------------------------------------------------------------------------------------ 7. the autograd surface
def leaves_of(dp=DP, dtype=torch.float64, device=DEV):
    return [torch.tensor(v, dtype=dtype, device=device, requires_grad=True) for v in dp[:3]]


def hand_dp(lens, img, alpha, z, scales, x2, y2, G, num, den, dp, wvln, photometric=False):
    """render_layers' gradient in (h, f, w) by hand for one wavelength: gnum and gden from the TOTAL sums, then
    layer_dp_grad_batch over the chunks of 64 samples, added in order -> [3] float64."""
    Wt = alpha.shape[-1] if alpha is not None else img.shape[-1]
    inv = [inv_texel_of(lens, s, Wt) for s in scales]
    gnum = gnum_from_image_grad(G, den, x2.shape[0], photometric).contiguous()
    gden = gden_from_image_grad(G, num, den, photometric)
    total = torch.zeros(3, dtype=torch.float64, device=DEV)
    for s0 in range(0, x2.shape[0], 64):
        xs, ys = x2[s0:s0 + 64], y2[s0:s0 + 64]
        out = layer_batch(lens, alpha, img, z, inv, xs, ys, dp, wvln)
        total += layer_dp_grad_batch(lens, alpha, img, z, inv, xs, ys, out["trips"], gnum, gden, dp, wvln)
    return total


def test_render_layers_backward_is_the_entry_run_by_hand(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        L, Ht, Wt = 3, 5, 9
        z = list(DEPTHS3)
        scales = [half_cover_scale(lens, d, lens.focus_depth) for d in z]
        alpha0 = alpha_stack(L, Ht, Wt, seed=61)
        img0 = texture(L * 3, Ht, Wt, seed=62).view(L, 3, Ht, Wt)
        G = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(64)).to(DEV)
        x2, y2 = pupil_points(lens, 128, seed=63)

        def run(img, spp, wvln=WVLN, pts=None, leaves=None, **kw):
            leaves = leaves_of() if leaves is None else leaves
            pts = (x2[:spp], y2[:spp]) if pts is None else pts
            views = lens.render_layers(img, alpha0, z, spp=spp, dp=(*leaves, DP[3]), wvln=wvln, scales=scales,
                                       pupil_points=pts, dp_grad=True, **kw)
            plain = lens.render_layers(img, alpha0, z, spp=spp, dp=DP, wvln=wvln, scales=scales, pupil_points=pts,
                                       return_sums=True, **kw)
            for v, p in zip(views, plain):
                assert torch.equal(v, p) and v.grad_fn is not None and p.grad_fn is None
            sum((v * G[n]).sum() for n, v in enumerate(views)).backward()
            return torch.stack([v.grad for v in leaves]), plain[2], plain[3]          # num, den

        # 128 samples: two chunks, both on the TOTAL num and den
        got, num, den = run(img0, 128)
        hand = hand_dp(lens, img0, alpha0, z, scales, x2, y2, G, num, den, DP, WVLN)
        print(f"128 spp: {got.tolist()}")
        assert got.dtype == torch.float64 and torch.equal(got, hand) and bool((got != 0).all())
        # photometric: no gden
        got, num, den = run(img0, 8, photometric=True)
        assert gden_from_image_grad(G, num, den, True) is None
        assert torch.equal(got, hand_dp(lens, img0, alpha0, z, scales, x2[:8], y2[:8], G, num, den, DP, WVLN, photometric=True))
        assert not torch.equal(got, run(img0, 8)[0])
        # per-channel wavelengths: the sum of three single-wavelength calls, a per-layer and a shared image
        xs, ys = zip(*(pupil_points(lens, 8, seed=64 + c) for c in range(3)))
        x3, y3 = torch.stack(xs), torch.stack(ys)
        for src in (img0, img0[1]):
            got, num, den = run(src, 8, wvln=WAVE_RGB, pts=(x3, y3))
            assert den.shape == (2, 3, H, W) and num.shape == (2, 3, H, W)
            total, calls = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
            for c in range(3):
                ch = (src[:, c:c + 1] if src.dim() == 4 else src[c:c + 1]).contiguous()
                total += hand_dp(lens, ch, alpha0, z, scales, x3[c], y3[c], G[:, c:c + 1], num[:, c:c + 1], den[:, c], DP,
                                 WAVE_RGB[c])
                one = leaves_of()
                vs = lens.render_layers(ch, alpha0, z, spp=8, dp=(*one, DP[3]), wvln=WAVE_RGB[c], scales=scales,
                                        pupil_points=(x3[c], y3[c]), dp_grad=True)
                sum((v * G[n, c:c + 1]).sum() for n, v in enumerate(vs)).backward()
                calls += torch.stack([v.grad for v in one])
            assert torch.equal(got, total) and torch.equal(got, calls)
        # h alone requires a gradient; r as a tensor gets none; fp32 leaves on the CPU get fp32 gradients there
        h = torch.tensor(DP[0], requires_grad=True)
        rr = torch.tensor(DP[3], requires_grad=True)
        vL, vR = lens.render_layers(img0, alpha0, z, spp=8, dp=(h, torch.tensor(DP[1]), DP[2], rr), wvln=WVLN, scales=scales,
                                    pupil_points=(x2[:8], y2[:8]), dp_grad=True)
        ((vL * G[0]).sum() + (vR * G[1]).sum()).backward()
        full = run(img0, 8)[0]
        assert h.grad is not None and h.grad.dtype == torch.float32 and h.grad.device.type == "cpu" and rr.grad is None
        # (the fp32 leaves' values differ from the float64 ones' in their last bits, and the gradient is rounded to fp32)
        assert abs(float(h.grad) - float(full[0])) <= 1e-3 * abs(float(full[0]))
        # dp_grad=False, and dp_grad=True under no_grad or without a tensor that requires one: the plain call
        kw = dict(spp=8, wvln=WVLN, scales=scales, pupil_points=(x2[:8], y2[:8]))
        ref = lens.render_layers(img0, alpha0, z, dp=DP, **kw)
        tens = tuple(torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in DP)
        off = lens.render_layers(img0, alpha0, z, dp=tens, **kw)
        with torch.no_grad():
            quiet = lens.render_layers(img0, alpha0, z, dp=tens, dp_grad=True, **kw)
        on = lens.render_layers(img0, alpha0, z, dp=DP, dp_grad=True, return_sums=True, **kw)
        for other in (off, quiet, on[:2]):
            assert all(torch.equal(a, b) and a.grad_fn is None for a, b in zip(other, ref))
        with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
            lens.render_layers(img0, alpha0, z, dp=tens, dp_grad=True, return_sums=True, **kw)
        with pytest.raises(ValueError, match="dp_grad=True with dp=None"):
            lens.render_layers(img0, alpha0, z, dp=None, dp_grad=True, **kw)


def test_dp_grad_and_scene_grad_compose(lens):
    """One backward runs both kernels from the one record.  h, f, w get what dp_grad alone gives them, bit for bit (a
    fixed summation order).  img and alpha get what scene_grad alone gives them within §7q's bound for two runs: that
    kernel adds with float64 atomics, whose sums depend on arrival order, so two runs of it are not the same bits
    whatever calls them (tests/test_gpu_render_layers_grad.py, test 7)."""
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        L, Ht, Wt = 3, 5, 9
        z = list(DEPTHS3)
        scales = [half_cover_scale(lens, d, lens.focus_depth) for d in z]
        alpha0 = alpha_stack(L, Ht, Wt, seed=61)
        img0 = texture(L * 3, Ht, Wt, seed=62).view(L, 3, Ht, Wt)
        G = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(65)).to(DEV)
        x2, y2 = pupil_points(lens, 8, seed=66)
        kw = dict(spp=8, wvln=WVLN, scales=scales, pupil_points=(x2, y2))

        def run(scene, dpg):
            img, alpha, leaves = img0.clone().requires_grad_(), alpha0.clone().requires_grad_(), leaves_of()
            vs = lens.render_layers(img, alpha, z, dp=(*leaves, DP[3]), scene_grad=scene, dp_grad=dpg, **kw)
            sum((v * G[n]).sum() for n, v in enumerate(vs)).backward()
            return img.grad, alpha.grad, [v.grad for v in leaves], vs

        gi_b, ga_b, gd_b, v_b = run(True, True)
        gi_s, ga_s, gd_s, v_s = run(True, False)
        gi_d, ga_d, gd_d, v_d = run(False, True)
        for a, b, c in zip(v_b, v_s, v_d):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert all(g is None for g in gd_s) and gi_d is None and ga_d is None
        assert all(torch.equal(a, b) for a, b in zip(gd_b, gd_d)) and all(bool(a != 0) for a in gd_b)
        den = lens.render_layers(img0, alpha0, z, dp=DP, return_sums=True, **kw)[3]
        ha, ht, ba, bt = hand_grads(lens, img0, alpha0, z, scales, x2, y2, G, den, DP, WVLN)
        for tag, both, alone, hand, bound in (("img", gi_b, gi_s, ht, bt), ("alpha", ga_b, ga_s, ha, ba)):
            assert_fp32_of(f"composed, {tag}", both, hand, bound)
            assert_fp32_of(f"scene_grad alone, {tag}", alone, hand, bound)
            print(f"{tag}: composed and alone are {'bit-equal' if torch.equal(both, alone) else 'not bit-equal'}")


def test_render_rgbd_backward_sums_the_batch(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        frame = texture(2 * 3, H, W, seed=71).view(2, 3, H, W)
        x2, y2 = pupil_points(lens, 8, seed=72)
        depth = torch.full((2, 1, H, W), -3000.0, device=DEV)
        depth[0, 0, :, 20:40] = -700.0
        depth[1, 0, 1:, 5:30] = -700.0
        zs = [-700.0, -3000.0]
        scales = [magnification(lens, d, lens.focus_depth) for d in zs]
        kw = dict(spp=8, wvln=WVLN, pupil_points=(x2, y2))
        G = torch.randn(2, 2, 3, H, W, generator=torch.Generator().manual_seed(73)).to(DEV)
        leaves = leaves_of()
        gL, gR = lens.render_rgbd(frame, depth, layer_depths=zs, scales=scales, dp=(*leaves, DP[3]), dp_grad=True, **kw)
        pL, pR = lens.render_rgbd(frame, depth, layer_depths=zs, scales=scales, dp=DP, **kw)
        assert torch.equal(gL, pL) and torch.equal(gR, pR) and gL.grad_fn is not None and pL.grad_fn is None
        ((gL * G[0]).sum() + (gR * G[1]).sum()).backward()
        got = torch.stack([v.grad for v in leaves])
        per_frame = []
        for b in range(2):
            alpha = layers_from_rgbd(depth[b, 0], zs)
            sums = lens.render_layers(frame[b], alpha, zs, scales=scales, dp=DP, return_sums=True, **kw)
            per_frame.append(hand_dp(lens, frame[b].contiguous(), alpha, zs, scales, x2, y2, G[:, b], sums[2], sums[3], DP, WVLN))
        print(f"render_rgbd: {got.tolist()} = {per_frame[0].tolist()} + {per_frame[1].tolist()}")
        assert torch.equal(got, per_frame[0] + per_frame[1]) and bool((per_frame[0] != 0).all())
        with pytest.raises(ValueError, match="dp_grad=True with dp=None"):
            lens.render_rgbd(frame, depth, layer_depths=zs, scales=scales, dp=None, dp_grad=True, **kw)


# ------------------------------------------------------------------------------------ 8. kernel against kernel
def test_a_central_difference_through_the_forward_kernel_on_the_occlusion_scene(lens):
    """The occlusion scene of test 5 of test_gpu_render_layers.py: an opaque half-plane at -700 mm in front of an
    opaque background at -3000 mm.  <G, num / den> of the FORWARD kernel at theta +- delta against the backward's
    gradient, theta = h, f, w.  The forward's weights are fp32 closed forms, held to 4 r^2 3.1e-7 absolute by
    test_gpu_render_layers.py; a central difference divides twice that by 2 delta per ray, and the model's second
    derivative jumps at every clamp edge a ray crosses between theta - delta and theta + delta, so the step's curvature
    term has no bound that could be written down without counting those crossings: the difference is
    printed next to the gradient, and the sign is asserted where the gradient exceeds the rounding term
    E_w sum_rays ra (sum_k |gnum_k c_k| + |gden|) / delta, E_w = 4 r^2 3.1e-7."""
    z = [-700.0, -3000.0]
    spp, delta = 8, 1e-3
    with sensor(lens, **SMALL):
        H, W = lens.sensor_res
        Ht, Wt = H, W
        scales = [magnification(lens, d, lens.focus_depth) for d in z]
        inv = [inv_texel_of(lens, s, Wt) for s in scales]
        alpha = torch.zeros(2, Ht, Wt, device=DEV)
        alpha[0, :, Wt // 2:] = 1.0
        alpha[1] = 1.0
        tex = torch.zeros(2, 2, Ht, Wt, device=DEV)
        tex[0, 0], tex[1, 1] = 1.0, 1.0
        x2, y2 = pupil_points(lens, spp, seed=51)
        G = torch.randn(2, 2, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(52)).to(DEV)

        def f(dp):
            out = layer_batch(lens, alpha, tex, z, inv, x2, y2, dp, WVLN)
            den = out["den"].unsqueeze(1)
            return float((G * torch.where(den > 0, out["num"] / den.clamp_min(1e-300), torch.zeros_like(out["num"]))).sum()), out

        f0, out = f(DP)
        gnum = gnum_from_image_grad(G, out["den"]).contiguous()
        gden = gden_from_image_grad(G, out["num"], out["den"])
        grad = layer_dp_grad_batch(lens, alpha, tex, z, inv, x2, y2, out["trips"], gnum, gden, DP, WVLN).cpu().numpy()
        # the rounding term: every |wr c| term of the sums, divided by its den, at the weights' absolute error
        absn = layer_batch(lens, alpha, tex, z, inv, x2, y2, None, WVLN)["num"][0]            # unit weights: sum ra c_k
        den = out["den"]
        per = (G.abs() * absn[None]).sum(1) / den.clamp_min(1e-300) + (G * out["num"]).abs().sum(1) / (den * den).clamp_min(1e-300)
        noise = 4 * DP[3] ** 2 * 3.1e-7 * float(torch.where(den > 0, per, torch.zeros_like(per)).sum()) / delta
        for j, name in enumerate("hfw"):
            hi, lo = list(DP), list(DP)
            hi[j], lo[j] = DP[j] + delta, DP[j] - delta
            cd = (f(tuple(hi))[0] - f(tuple(lo))[0]) / (2 * delta)
            print(f"d<G, image>/d{name}: backward {grad[j]:+.6e}, central difference {cd:+.6e}, difference {cd - grad[j]:+.3e}, "
                  f"rounding term {noise:.3e}")
            assert np.isfinite(cd) and np.isfinite(grad[j])
            if abs(grad[j]) > 2 * noise:
                assert np.sign(cd) == np.sign(grad[j]), (name, cd, grad[j])
        assert np.abs(grad).max() > 0


# ------------------------------------------------------------------------------------ 9. refusals
def test_the_entry_refuses_and_leaves_partial_at_its_poison(lens, rays):
    spp, planes, Ht, Wt, L = 8, 5, 2, 3, 3
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = (int(v) for v in lens.sensor_res)
        rows = (H * W + 255) // 256
        alpha = alpha_stack(L, Ht, Wt)
        tex = texture(L * planes, Ht, Wt, seed=82).view(L, planes, Ht, Wt)
        inv = layer_inv_texels(lens, depths, Wt)
        gnum, gden = seeded_gnum(2, planes, H, W, seed=83), seeded_gden(H, W, seed=84)
        x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
        fwd = layer_batch(lens, alpha, tex, depths, inv, x2, y2, DP, WVLN)
        partial, p_ok = _guarded(2 * rows * 3, torch.float64)
        partial.fill_(POISON)
        lib = _lib.lib()

        def refused(msg, *a, **k):
            assert _call_entry(lens, x2, y2, *a, **k) != 0
            assert msg in lib.sdirt_last_error(), lib.sdirt_last_error()

        ok = (fwd["trips"], alpha, tex, depths, inv, gnum, gden, partial, None)
        refused(b"null argument", *ok[:5], None, gden, partial, None)                       # gnum
        refused(b"null argument", *ok[:7], None, None)                                       # partial
        refused(b"null dp", *ok, dp=None)
        refused(b"dp->r must be > 0", *ok, dp=(0.78, 1.44, 0.3, 0.0))
        refused(b"dp->r must be > 0", *ok, dp=(0.78, 1.44, 0.3, -0.5))
        refused(b"dp->f must differ from dp->h", *ok, dp=(0.78, 0.78, 0.3, 0.5))
        refused(b"negative layer stride", *ok, stride=-1)
        for bad in ([-400.0, -400.0, -20000.0], [-400.0, -300.0, -20000.0], [400.0, -1000.0, -2000.0]):
            refused(b"strictly descending", fwd["trips"], alpha, tex, bad, inv, gnum, gden, partial, None)
        bad_trips = fwd["trips"].copy()
        bad_trips[0] = 99
        refused(b"trips[0]", bad_trips, *ok[1:])
        dpp = C.byref(_lib.DpParams(*DP))
        for n_layers in (0, 17):
            rc = lib.sdirt_render_layers_dp_grad(lens.dev_lens(WVLN), None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum),
                                                 dptr(gnum), 0.0, 1, 1, 1, dpp, n_layers, (C.c_double * 17)(),
                                                 (C.c_double * 17)(), dptr(alpha), dptr(tex), 0, 1, Ht, Wt, dptr(gnum),
                                                 dptr(gden), dptr(partial), None, stream_ptr(lens.device))
            assert rc != 0 and b"SDIRT_MAX_LAYERS" in lib.sdirt_last_error()
        rc = lib.sdirt_render_layers_dp_grad(lens.dev_lens(WVLN), None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum), dptr(gnum),
                                             0.0, 0, 1, 1, dpp, 1, (C.c_double * 1)(-1.0), (C.c_double * 1)(1.0), dptr(alpha),
                                             dptr(tex), 0, 1, Ht, Wt, dptr(gnum), dptr(gden), dptr(partial), None,
                                             stream_ptr(lens.device))
        assert rc != 0 and b"at least 1" in lib.sdirt_last_error()
        rc = lib.sdirt_render_layers_dp_grad(None, None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum), dptr(gnum), 0.0, 1, 1, 1,
                                             dpp, 1, (C.c_double * 1)(-1.0), (C.c_double * 1)(1.0), dptr(alpha), dptr(tex), 0,
                                             1, Ht, Wt, dptr(gnum), dptr(gden), dptr(partial), None, stream_ptr(lens.device))
        assert rc != 0 and b"null lens" in lib.sdirt_last_error()
        torch.cuda.synchronize()
        assert bool((partial == POISON).all()) and p_ok()
        # ... and the same arguments, unrefused, overwrite every element
        assert _call_entry(lens, x2, y2, *ok) == 0
        torch.cuda.synchronize()
        assert not bool((partial == POISON).any()) and p_ok()
