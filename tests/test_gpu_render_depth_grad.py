"""k_render_layers_depth_grad (csrc/sdirt_render_rt.hip) on the GPU: the layered render's backward into
the layer depths and the layers' texel scales -- the forward's rays again, every lookup's derivative in its landing
point times the ray's slope, pushed through §7q's compositing adjoint, one row of 2 L float64 sums per workgroup.

  1. ray_dir is the staged chain's direction after trace, bit for bit, dead rays included;
  2. the kernel against tests/render_depth_grad_f64.py (written from the text of §7s) on the forward's own landing
     record and the kernel's own ray_dir, §7q's thirteen stacks, within 2 (n + rho) 2^-53 sum|term|;
  3. all 24 instantiations;
  4. plane groups: 5 and 9 planes;
  5. a null alpha, alpha == 1 and render_plane(depth_grad=True), bit for bit; NaN textures behind an opaque stack;
  6. the same bits: two runs, a side stream, partial overwritten, guard bands, the entry's refusals;
  7. the autograd surface of render_layers, render_rgbd and render_plane;
  8. kernel against kernel: a central difference through the FORWARD kernel in one z_l;
  9. physics: the depth gradient of the dual-pixel disparity changes sign across focus.

No atomics: what the kernel adds up IS asserted bit-equal from run to run.  Sensors, textures and the seeded alpha stacks
are those of test_gpu_render_layers.py, test_gpu_render_layers_grad.py and test_gpu_render_raytraced_edges.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_depth_grad_f64 as RZ
from render_rt_f64 import tap_origin
from test_gpu_render_dp_grad import NARROW
from test_gpu_render_layers import (CASES_3, DEPTHS3, alpha_stack, land_points, layer_inv_texels, lens, rays,  # noqa: F401
                                    stack_depths)
from test_gpu_render_layers_grad import TINY, assert_fp32_of, hand_grads, seeded_gnum, stopped_with_something_behind
from test_gpu_render_raytraced import DP, DP_BIG, DEV, SMALL, WIDE, WVLN, pupil_points, sensor
from test_gpu_render_raytraced_edges import RAGGED, _guarded, half_cover_scale, inv_texel_of, magnification, texture

from sdirt_amd import _lib
from sdirt_amd.basics import WAVE_RGB, Ray, dptr, stream_ptr
from sdirt_amd.render_rt import (gnum_from_image_grad, layer_batch, layer_depth_grad_batch, layers_from_rgbd, sensor_axes)

pytestmark = pytest.mark.gpu
FLOOR = 0.05
POISON = -7.0


def mixed_alpha(L, Ht, Wt, seed=11, back=0.5):
    """alpha_stack's seeded binary coverage with three texels in ten made fractional (0.25 .. 1): rays read exact zeros
    and ones (an opaque texel stops them) as well as transitions, where the coverage has a derivative."""
    a = alpha_stack(L, Ht, Wt, seed=seed, back=back)
    g = torch.Generator().manual_seed(seed + 1000)
    frac = (0.25 + 0.75 * torch.rand(L, Ht, Wt, generator=g)).to(DEV)
    pick = (torch.rand(L, Ht, Wt, generator=g) < 0.3).to(DEV)
    return torch.where(pick, frac, a)


def reference(land, rd, L, V, alpha, tex, inv, gnum):
    """The restatement of §7s on a launch's landing record and the kernel's ray_dir record."""
    lx, ly = land_points(land, L)
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return RZ.depth_grads_f64(cpu(lx), cpu(ly), cpu(land[0]), cpu(land[1:1 + V]), cpu(rd), cpu(alpha), cpu(tex), inv, cpu(gnum))


def assert_grad(tag, got, ref, L):
    """[L, 2] of the kernel against the restatement: every layer, both components, within §7s's bound."""
    got = got.cpu().numpy()
    assert got.shape == (L, 2) and got.dtype == np.float64
    tol = RZ.bound(ref["n"], L, ref["abs"].T).T
    err = np.abs(got - ref["grad"])
    print(f"{tag}: gdepth {got[:, 0]}, worst |kernel - f64| / bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}, n {ref['n'].tolist()}")
    assert (err <= tol).all(), err / np.maximum(tol, 1e-300)
    assert np.isfinite(got).all()


def forward_and_grad(lens, alpha, tex, depths, inv, x2, y2, dp, gnum):
    out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, dp, WVLN, landing=True)
    grad, rd = layer_depth_grad_batch(lens, alpha, tex, depths, inv, x2, y2, out["trips"], gnum, dp, WVLN, ray_dir=True)
    assert grad.shape == (len(depths), 2) and grad.dtype == torch.float64
    assert rd.shape == (3,) + tuple(x2.shape) and rd.dtype == torch.float32
    return out, grad, rd


# ------------------------------------------------------------------------------------ 1. ray_dir
def staged_directions(lens, x2, y2):
    """The staged chain on the pupil points: Ray(o, o2 - o), trace (backward) -> (dx, dy, dz) [3, S, H, W], ra."""
    x1, y1 = sensor_axes(lens, True)
    gx, gy = torch.meshgrid(x1, y1, indexing="xy")
    o = torch.stack((gx, gy, torch.full_like(gx, lens.d_sensor)), 2)
    o2 = torch.stack((x2, y2, torch.full_like(x2, lens.exit_pupil()[0])), -1)
    ray = Ray(torch.broadcast_to(o, o2.shape), o2 - o, wvln=WVLN, device=lens.device)
    shape, n = ray.shape, ray.numel
    ray, _, _ = lens.trace(ray)
    return torch.stack([ray.soa[c, :n].view(shape).clone() for c in (3, 4, 5)]), ray.soa[6, :n].view(shape).clone()


@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_ray_dir_is_the_staged_chain_s_direction_after_trace(lens, precision):
    spp, L, Ht, Wt = 8, 3, 5, 9
    depths = list(DEPTHS3)
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        x2, y2 = pupil_points(lens, spp, seed=301)
        d, ra = staged_directions(lens, x2, y2)
        inv = layer_inv_texels(lens, depths, Wt)
        out, _, rd = forward_and_grad(lens, mixed_alpha(L, Ht, Wt), texture(2, Ht, Wt, seed=302), depths, inv, x2, y2, DP,
                                      seeded_gnum(2, 2, H, W, seed=303))
        dead = ra == 0
        assert torch.equal(out["landing"][0], ra) and 0.01 < float(dead.float().mean()) < 0.9
        # bit for bit, NaN for NaN: dead rays included
        assert torch.equal(rd.view(torch.int32), d.view(torch.int32))
        assert bool(torch.isfinite(rd[:, ~dead]).all()) and bool((rd[2, ~dead] < 0).all())


# ------------------------------------------------------------------------------------ 2. against the restatement
@pytest.mark.parametrize("dp", [DP, None], ids=["dp", "one-view"])
@pytest.mark.parametrize("L, shape, spp, shared, planes, back", CASES_3 + TINY)
def test_gradient_equals_the_float64_restatement(lens, rays, L, shape, spp, shared, planes, back, dp):
    Ht, Wt = shape
    V = 1 if dp is None else 2
    depths = stack_depths(L)
    r = rays(spp, depths)
    tag = f"L {L}, {Ht} x {Wt}, spp {spp}, {'shared' if shared else 'per-layer'}, {planes} planes, V {V}"
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        assert H * W > 256 and (H * W) % 64 != 0                 # several workgroups, a ragged last wave
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = mixed_alpha(L, Ht, Wt, seed=23, back=back)      # a seed whose 2 x 3 stacks have an opaque edge column
        tex = texture(planes, Ht, Wt, seed=31) if shared else texture(L * planes, Ht, Wt, seed=32).view(L, planes, Ht, Wt)
        gnum = seeded_gnum(V, planes, H, W, seed=33)
        out, grad, rd = forward_and_grad(lens, alpha, tex, depths, inv, r["x2"], r["y2"], dp, gnum)
        ref = reference(out["landing"], rd, L, V, alpha, tex, inv, gnum)
        assert_grad(tag, grad, ref, L)
        live = out["landing"][0].cpu().numpy() != 0
        outside = ((ref["c0"] < 0) | (ref["c0"] >= Wt - 1)) & live[None]
        assert (ref["Pu"][outside] == 0).all()                   # both columns are one texel: exactly 0
        shares = dict(coverage=float((ref["cov_u"] != 0).any(0)[live].mean()), colour=float((ref["col_u"] != 0).any(0)[live].mean()),
                      outside=float(outside.any(0)[live].mean()),
                      stopped=stopped_with_something_behind(ref, out["landing"][0]) if L > 1 else None)
        print(f"{tag}: shares of the live rays {shares}")
        if min(Ht, Wt) > 1:
            # conditions on the inputs, read off the forward's record
            assert shares["coverage"] >= FLOOR and shares["colour"] >= FLOOR and shares["outside"] >= FLOOR, shares
            assert L == 1 or shares["stopped"] >= FLOOR, shares
            assert (ref["grad"] != 0).all() and (ref["abs"] > 0).all()
        else:
            # a 1-texel extent: no derivative along it, and the whole gradient is 0 where both extents are 1
            assert Wt > 1 or (ref["Pu"] == 0).all()
            assert Ht > 1 or (ref["Pv"] == 0).all()
            assert max(Ht, Wt) > 1 or not bool(grad.any())


# ------------------------------------------------------------------------------------ 3. every instantiation
@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("dp", [None, DP, DP_BIG], ids=["none", "small", "big"])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_gradient_of_every_instantiation(lens, precision, dp, planes):
    """k_render_layers_depth_grad<M, DP, NT>: 2 x 3 x 4, at L = 2, each against the landing record of its own forward."""
    spp, Ht, Wt, L = 5, 7, 12, 2
    V = 1 if dp is None else 2
    depths = stack_depths(L)
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        x2, y2 = pupil_points(lens, spp, seed=311)
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = mixed_alpha(L, Ht, Wt, seed=41)
        tex = texture(L * 4, Ht, Wt, seed=42).view(L, 4, Ht, Wt)[:, :planes].contiguous()
        gnum = seeded_gnum(V, planes, H, W, seed=43)
        out, grad, rd = forward_and_grad(lens, alpha, tex, depths, inv, x2, y2, dp, gnum)
        ref = reference(out["landing"], rd, L, V, alpha, tex, inv, gnum)
        assert_grad(f"{precision}, dp {dp}, {planes} planes", grad, ref, L)
        assert (ref["grad"] != 0).all()


# ------------------------------------------------------------------------------------ the C entry, directly
def _call_entry(lens, x2, y2, trips, alpha, tex, depths, inv, gnum, partial, rd, dp=DP, stride=None, stream=None):
    H, W = (int(v) for v in lens.sensor_res)
    K, L = len(lens.surfaces), len(depths)
    T, Ht, Wt = (int(v) for v in tex.shape[-3:])
    V = 1 if dp is None else 2
    spp = int(x2.shape[0])
    x1, y1 = sensor_axes(lens, True)
    assert x2.shape == (spp, H, W) and x2.dtype == torch.float32 and x2.is_contiguous() and y2.is_contiguous()
    assert tex.is_contiguous() and (alpha is None or alpha.is_contiguous()) and 1 <= L <= _lib.MAX_LAYERS
    assert gnum is None or (gnum.shape == (V, T, H, W) and gnum.dtype == torch.float64 and gnum.is_contiguous())
    assert partial is None or (partial.dtype == torch.float64
                               and partial.numel() == ((T + 3) // 4) * ((H * W + 255) // 256) * L * 2)
    assert rd is None or (rd.dtype == torch.float32 and rd.numel() == 3 * spp * H * W)
    pupilz, _ = lens.exit_pupil()
    dpp = None if dp is None else C.byref(_lib.DpParams(*(float(v) for v in dp)))
    stride = (T * Ht * Wt if tex.dim() == 4 else 0) if stride is None else stride
    return _lib.lib().sdirt_render_layers_depth_grad(
        lens.dev_lens(WVLN), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
        float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), spp, H, W, dpp, L, (C.c_double * L)(*depths),
        (C.c_double * L)(*inv), dptr(alpha), dptr(tex), stride, T, Ht, Wt, dptr(gnum), dptr(partial), dptr(rd),
        stream_ptr(lens.device) if stream is None else stream)


# ------------------------------------------------------------------------------------ 4. plane groups
@pytest.mark.parametrize("planes", [5, 9])
def test_plane_groups_are_slices_of_partial(lens, rays, planes):
    """More than four planes run as further launches: every group of four planes writes a leading slice of `partial`
    of its own, equal in every bit to a call on those planes alone, and the whole is the restatement on all planes."""
    spp, L, Ht, Wt = 5, 3, 5, 9
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = (int(v) for v in lens.sensor_res)
        rows, groups = (H * W + 255) // 256, (planes + 3) // 4
        assert groups == {5: 2, 9: 3}[planes] and rows == 3
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = mixed_alpha(L, Ht, Wt, seed=45)
        tex = texture(L * planes, Ht, Wt, seed=46).view(L, planes, Ht, Wt)
        gnum = seeded_gnum(2, planes, H, W, seed=47)
        x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
        out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, DP, WVLN, landing=True)
        partial = torch.full((groups, rows, L, 2), POISON, dtype=torch.float64, device=DEV)
        rd = torch.empty(3, spp, H, W, dtype=torch.float32, device=DEV)
        assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, partial, rd) == 0
        torch.cuda.synchronize()
        total = torch.zeros(L, 2, dtype=torch.float64, device=DEV)
        for g in range(groups):
            sl = slice(4 * g, min(4 * g + 4, planes))
            alone = layer_depth_grad_batch(lens, alpha, tex[:, sl].contiguous(), depths, inv, x2, y2, out["trips"],
                                           gnum[:, sl].contiguous(), DP, WVLN)
            assert torch.equal(partial[g].sum(0), alone)
            assert_grad(f"{planes} planes, group {g}", partial[g].sum(0), reference(out["landing"], rd, L, 2, alpha,
                                                                                    tex[:, sl], inv, gnum[:, sl]), L)
            total += alone
        whole = reference(out["landing"], rd, L, 2, alpha, tex, inv, gnum)
        assert_grad(f"{planes} planes, all groups", partial.view(-1, L, 2).sum(0), whole, L)
        grad = layer_depth_grad_batch(lens, alpha, tex, depths, inv, x2, y2, out["trips"], gnum, DP, WVLN)
        assert torch.equal(grad, partial.view(-1, L, 2).sum(0))
        assert (np.abs(total.cpu().numpy() - whole["grad"]) <= 2 * RZ.bound(whole["n"], L, whole["abs"].T).T).all()


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
        gnum = seeded_gnum(2, planes, H, W, seed=62)
        x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
        out, grad, rd = forward_and_grad(lens, ones, tex, [depth], inv, x2, y2, DP, gnum)
        assert_grad("alpha == 1", grad, reference(out["landing"], rd, 1, 2, ones, tex, inv, gnum), 1)
        null = layer_depth_grad_batch(lens, None, tex, [depth], inv, x2, y2, out["trips"], gnum, DP, WVLN)
        assert torch.equal(null, grad) and bool((grad != 0).all())
        # render_plane(depth_grad=True): img [1, C, Ht, Wt], the loss sum_v <G_v, view_v>; depth and scale 0-d leaves
        z = torch.tensor(depth, dtype=torch.float64, device=DEV, requires_grad=True)
        sc = torch.tensor(scale, dtype=torch.float64, requires_grad=True)                     # on the CPU
        G = torch.randn(2, 1, planes, H, W, generator=torch.Generator().manual_seed(64)).to(DEV)
        kw = dict(spp=spp, wvln=WVLN, pupil_points=(x2, y2), dp=DP)
        vL, vR = lens.render_plane(tex[None], z, scale=sc, depth_grad=True, **kw)
        plain = lens.render_plane(tex[None], depth, scale=scale, return_sums=True, **kw)
        assert torch.equal(vL, plain[0]) and torch.equal(vR, plain[1]) and vL.grad_fn is not None and plain[0].grad_fn is None
        ((vL * G[0]).sum() + (vR * G[1]).sum()).backward()
        gn = gnum_from_image_grad(G[:, 0], plain[3]).contiguous()
        hand = layer_depth_grad_batch(lens, None, tex, [depth], inv, x2, y2, out["trips"], gn, DP, WVLN)
        mine = layer_depth_grad_batch(lens, ones, tex, [depth], inv, x2, y2, out["trips"], gn, DP, WVLN)
        print(f"render_plane(depth_grad=True): d/ddepth {float(z.grad):+.6e}, d/dscale {float(sc.grad):+.6e}")
        assert z.grad.shape == () and z.grad.dtype == torch.float64 and z.grad.device.type == "cuda"
        assert sc.grad.shape == () and sc.grad.device.type == "cpu"
        assert torch.equal(hand, mine) and float(z.grad) == float(hand[0, 0]) != 0
        assert float(sc.grad) == float(hand[0, 1]) * (-inv[0] / scale) != 0


def test_nothing_behind_an_opaque_stack_is_read_whatever_it_holds(lens, rays):
    """A null alpha: the ray meets layer 0 with a = 1, T = 0 behind it, and there is no coverage adjoint that would need
    the layers behind.  Their textures are NaN, and the gradient is the finite one of layer 0 alone, bit for bit; the
    layers behind get exact zeros."""
    spp, L, Ht, Wt, planes = 5, 3, 5, 9, 2
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        tex = texture(L * planes, Ht, Wt, seed=67).view(L, planes, Ht, Wt).clone()
        gnum = seeded_gnum(2, planes, H, W, seed=68)
        x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
        trips = layer_batch(lens, torch.ones(L, Ht, Wt, device=DEV), tex, depths, inv, x2, y2, DP, WVLN)["trips"]
        clean = layer_depth_grad_batch(lens, None, tex, depths, inv, x2, y2, trips, gnum, DP, WVLN)
        first = layer_depth_grad_batch(lens, None, tex[:1].contiguous(), depths[:1], inv[:1], x2, y2, trips, gnum, DP, WVLN)
        tex[1:] = float("nan")
        grad = layer_depth_grad_batch(lens, None, tex, depths, inv, x2, y2, trips, gnum, DP, WVLN)
        assert bool(torch.isfinite(grad).all()) and torch.equal(grad, clean) and torch.equal(grad[:1], first)
        assert not bool(grad[1:].any()) and bool((grad[0] != 0).all())


# ------------------------------------------------------------------------------------ 6. the same bits, guards, refusals
@pytest.mark.parametrize("sens, tail", [(RAGGED, 193), (NARROW, 133)], ids=["ragged", "narrow"])
def test_two_runs_and_a_side_stream_give_the_same_bits_inside_guard_bands(lens, sens, tail):
    """The entry directly: partial and ray_dir are slices between guard bands; partial, poisoned with -7, is overwritten
    in every element; a second run and a run on a side stream give the same bits.  The last workgroup holds live pixels
    and lanes past the sensor -- on the narrow sensor a whole wave of them, which must still hand its zeros to the
    workgroup's sum.  L = 16: 128 KB of dynamic LDS, above the default allowance."""
    spp, L, Ht, Wt, planes = 5, 16, 5, 141, 3
    depths = stack_depths(L)
    with sensor(lens, **sens):
        H, W = (int(v) for v in lens.sensor_res)
        rows = (H * W + 255) // 256
        assert rows == 3 and H * W - 256 * (rows - 1) == tail and (H * W) % 64 != 0
        x2, y2 = pupil_points(lens, spp, seed=86)
        alpha, tex = mixed_alpha(L, Ht, Wt, back=0.2), texture(planes, Ht, Wt, seed=83)
        inv = layer_inv_texels(lens, depths, Wt)
        gnum = seeded_gnum(2, planes, H, W, seed=84)
        out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, DP, WVLN, landing=True)
        runs = []
        for n in range(3):
            partial, p_ok = _guarded(rows * L * 2, torch.float64)
            rd, r_ok = _guarded(3 * spp * H * W, torch.float32)
            partial.fill_(POISON)
            if n < 2:
                assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, partial, rd) == 0
            else:
                side = torch.cuda.Stream(DEV)
                side.wait_stream(torch.cuda.current_stream(DEV))
                with torch.cuda.stream(side):
                    assert torch.cuda.current_stream(DEV) == side
                    assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, partial, rd,
                                       stream=stream_ptr(lens.device)) == 0
                side.synchronize()
            torch.cuda.synchronize()
            assert p_ok() and r_ok()
            assert not bool((partial == POISON).any()) and bool(torch.isfinite(partial).all())
            assert bool((partial.view(rows, L, 2)[-1, 0] != 0).all())            # the last workgroup's live pixels count
            runs.append((partial.clone(), rd.clone()))
        for p, x in runs[1:]:
            assert torch.equal(p, runs[0][0]) and torch.equal(x.view(torch.int32), runs[0][1].view(torch.int32))
        rd = runs[0][1].view(3, spp, H, W)
        ref = reference(out["landing"], rd, L, 2, alpha, tex, inv, gnum)
        assert_grad("guarded", runs[0][0].view(rows, L, 2).sum(0), ref, L)
        # a null ray_dir: the same rows
        partial = torch.full((rows, L, 2), POISON, dtype=torch.float64, device=DEV)
        assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gnum, partial, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(partial.view(-1), runs[0][0])
        # a row is its workgroup's 256 pixels alone: the adjoints of the last workgroup's pixels zeroed, its row is 0
        gn0 = gnum.clone()
        gn0.view(2, planes, -1)[..., 512:] = 0
        assert _call_entry(lens, x2, y2, out["trips"], alpha, tex, depths, inv, gn0, partial, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(partial[:2].reshape(-1), runs[0][0][:2 * L * 2]) and not bool(partial[2].any())
        # ... and the last row alone is the restatement on the last workgroup's pixels
        gn1 = gnum.clone()
        gn1.view(2, planes, -1)[..., :512] = 0
        assert_grad(f"the last workgroup's {tail} pixels", runs[0][0].view(rows, L, 2)[2],
                    reference(out["landing"], rd, L, 2, alpha, tex, inv, gn1), L)


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
        gnum = seeded_gnum(2, planes, H, W, seed=83)
        x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
        fwd = layer_batch(lens, alpha, tex, depths, inv, x2, y2, DP, WVLN)
        partial, p_ok = _guarded(2 * rows * L * 2, torch.float64)
        partial.fill_(POISON)
        lib = _lib.lib()

        def refused(msg, *a, **k):
            assert _call_entry(lens, x2, y2, *a, **k) != 0
            assert msg in lib.sdirt_last_error(), lib.sdirt_last_error()

        ok = (fwd["trips"], alpha, tex, depths, inv, gnum, partial, None)
        refused(b"null argument", *ok[:5], None, partial, None)                              # gnum
        refused(b"null argument", *ok[:6], None, None)                                       # partial
        refused(b"negative layer stride", *ok, stride=-1)
        for bad in ([-400.0, -400.0, -20000.0], [-400.0, -300.0, -20000.0], [400.0, -1000.0, -2000.0]):
            refused(b"strictly descending", fwd["trips"], alpha, tex, bad, inv, gnum, partial, None)
        bad_trips = fwd["trips"].copy()
        bad_trips[0] = 99
        refused(b"trips[0]", bad_trips, *ok[1:])
        dpp = C.byref(_lib.DpParams(*DP))
        for n_layers in (0, 17):
            rc = lib.sdirt_render_layers_depth_grad(lens.dev_lens(WVLN), None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum),
                                                    dptr(gnum), 0.0, 1, 1, 1, dpp, n_layers, (C.c_double * 17)(),
                                                    (C.c_double * 17)(), dptr(alpha), dptr(tex), 0, 1, Ht, Wt, dptr(gnum),
                                                    dptr(partial), None, stream_ptr(lens.device))
            assert rc != 0 and b"SDIRT_MAX_LAYERS" in lib.sdirt_last_error()
        rc = lib.sdirt_render_layers_depth_grad(lens.dev_lens(WVLN), None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum),
                                                dptr(gnum), 0.0, 0, 1, 1, dpp, 1, (C.c_double * 1)(-1.0), (C.c_double * 1)(1.0),
                                                dptr(alpha), dptr(tex), 0, 1, Ht, Wt, dptr(gnum), dptr(partial), None,
                                                stream_ptr(lens.device))
        assert rc != 0 and b"at least 1" in lib.sdirt_last_error()
        rc = lib.sdirt_render_layers_depth_grad(None, None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum), dptr(gnum), 0.0, 1, 1,
                                                1, dpp, 1, (C.c_double * 1)(-1.0), (C.c_double * 1)(1.0), dptr(alpha), dptr(tex),
                                                0, 1, Ht, Wt, dptr(gnum), dptr(partial), None, stream_ptr(lens.device))
        assert rc != 0 and b"null lens" in lib.sdirt_last_error()
        torch.cuda.synchronize()
        assert bool((partial == POISON).all()) and p_ok()
        # ... and the same arguments, unrefused, overwrite every element
        assert _call_entry(lens, x2, y2, *ok) == 0
        torch.cuda.synchronize()
        assert not bool((partial == POISON).any()) and p_ok()


# ------------------------------------------------------------------------------------ 7. the autograd surface
def hand_depth(lens, img, alpha, z, scales, x2, y2, G, den, dp, wvln, photometric=False):
    """render_layers' gradient in (depths, inv_texels) by hand for one wavelength: gnum from the TOTAL den, then
    layer_depth_grad_batch over the chunks of 64 samples, added in order -> [L, 2] float64, and the inv_texels."""
    Wt = alpha.shape[-1] if alpha is not None else img.shape[-1]
    inv = [inv_texel_of(lens, s, Wt) for s in scales]
    gnum = gnum_from_image_grad(G, den, x2.shape[0], photometric).contiguous()
    total = torch.zeros(len(z), 2, dtype=torch.float64, device=DEV)
    for s0 in range(0, x2.shape[0], 64):
        xs, ys = x2[s0:s0 + 64], y2[s0:s0 + 64]
        out = layer_batch(lens, alpha, img, z, inv, xs, ys, dp, wvln)
        total += layer_depth_grad_batch(lens, alpha, img, z, inv, xs, ys, out["trips"], gnum, dp, wvln)
    return total, inv


def to_scales(hand, inv, scales):
    """The chain from inv_texel to scale: -inv / scale."""
    return hand[:, 1] * torch.tensor([-v / s for v, s in zip(inv, scales)], dtype=torch.float64, device=DEV)


def test_render_layers_backward_is_the_entry_run_by_hand(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        L, Ht, Wt = 3, 5, 9
        z = list(DEPTHS3)
        scales = [half_cover_scale(lens, d, lens.focus_depth) for d in z]
        alpha0 = mixed_alpha(L, Ht, Wt, seed=61)
        img0 = texture(L * 3, Ht, Wt, seed=62).view(L, 3, Ht, Wt)
        G = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(64)).to(DEV)
        x2, y2 = pupil_points(lens, 70, seed=63)

        def leaves(dtype=torch.float64, device=DEV):
            return (torch.tensor(z, dtype=dtype, device=device, requires_grad=True),
                    torch.tensor(scales, dtype=dtype, device=device, requires_grad=True))

        def run(img, spp, wvln=WVLN, pts=None, zl=None, **kw):
            zt, st = leaves() if zl is None else zl
            pts = (x2[:spp], y2[:spp]) if pts is None else pts
            views = lens.render_layers(img, alpha0, zt, spp=spp, dp=DP, wvln=wvln, scales=st, pupil_points=pts,
                                       depth_grad=True, **kw)
            plain = lens.render_layers(img, alpha0, z, spp=spp, dp=DP, wvln=wvln, scales=scales, pupil_points=pts,
                                       return_sums=True, **kw)
            for v, p in zip(views, plain):
                assert torch.equal(v, p) and v.grad_fn is not None and p.grad_fn is None
            sum((v * G[n]).sum() for n, v in enumerate(views)).backward()
            return zt.grad, st.grad, plain[3]                                                # den

        # 70 samples: two chunks, both on the TOTAL den
        gz, gs, den = run(img0, 70)
        hand, inv = hand_depth(lens, img0, alpha0, z, scales, x2, y2, G, den, DP, WVLN)
        print(f"70 spp: d/ddepths {gz.tolist()}, d/dscales {gs.tolist()}")
        assert gz.dtype == torch.float64 and gz.shape == (L,) and torch.equal(gz, hand[:, 0]) and bool((gz != 0).all())
        assert torch.equal(gs, to_scales(hand, inv, scales)) and bool((gs != 0).all())
        one_chunk, _ = hand_depth(lens, img0, alpha0, z, scales, x2[:64], y2[:64], G, den, DP, WVLN)
        assert not torch.equal(one_chunk, hand)
        # photometric
        gz, gs, den = run(img0, 8, photometric=True)
        hand, _ = hand_depth(lens, img0, alpha0, z, scales, x2[:8], y2[:8], G, den, DP, WVLN, photometric=True)
        assert torch.equal(gz, hand[:, 0]) and not torch.equal(gz, run(img0, 8)[0])
        # per-channel wavelengths: the sum of three single-wavelength calls, a per-layer and a shared image
        xs, ys = zip(*(pupil_points(lens, 8, seed=64 + c) for c in range(3)))
        x3, y3 = torch.stack(xs), torch.stack(ys)
        for src in (img0, img0[1]):
            gz, gs, den = run(src, 8, wvln=WAVE_RGB, pts=(x3, y3))
            assert den.shape == (2, 3, H, W)
            total, calls = torch.zeros(L, 2, dtype=torch.float64, device=DEV), torch.zeros(L, dtype=torch.float64, device=DEV)
            for c in range(3):
                ch = (src[:, c:c + 1] if src.dim() == 4 else src[c:c + 1]).contiguous()
                total += hand_depth(lens, ch, alpha0, z, scales, x3[c], y3[c], G[:, c:c + 1], den[:, c], DP, WAVE_RGB[c])[0]
                zt, st = leaves()
                vs = lens.render_layers(ch, alpha0, zt, spp=8, dp=DP, wvln=WAVE_RGB[c], scales=st,
                                        pupil_points=(x3[c], y3[c]), depth_grad=True)
                sum((v * G[n, c:c + 1]).sum() for n, v in enumerate(vs)).backward()
                calls += zt.grad
            assert torch.equal(gz, total[:, 0]) and torch.equal(gz, calls)
        # scales built from the depths (a pinhole: scale = -k depth): autograd chains the two
        zt = torch.tensor(z, dtype=torch.float64, device=DEV, requires_grad=True)
        k = torch.tensor([-s / d for s, d in zip(scales, z)], dtype=torch.float64, device=DEV)
        built = -k * zt
        assert built.tolist() == scales
        vs = lens.render_layers(img0, alpha0, zt, spp=8, dp=DP, wvln=WVLN, scales=built, pupil_points=(x2[:8], y2[:8]),
                                depth_grad=True)
        sum((v * G[n]).sum() for n, v in enumerate(vs)).backward()
        gz, gs, _ = run(img0, 8)
        assert torch.equal(zt.grad, gz + gs * (-k))
        # depths alone require a gradient; fp32 leaves on the CPU get fp32 gradients there
        z32 = torch.tensor(z, requires_grad=True)
        vs = lens.render_layers(img0, alpha0, z32, spp=8, dp=DP, wvln=WVLN, scales=scales, pupil_points=(x2[:8], y2[:8]),
                                depth_grad=True)
        sum((v * G[n]).sum() for n, v in enumerate(vs)).backward()
        assert z32.grad.dtype == torch.float32 and z32.grad.device.type == "cpu" and torch.equal(z32.grad, gz.float().cpu())
        # dp=None: one view
        zt, st = leaves()
        one = lens.render_layers(img0, alpha0, zt, spp=8, dp=None, wvln=WVLN, scales=st, pupil_points=(x2[:8], y2[:8]),
                                 depth_grad=True)
        (one * G[0]).sum().backward()
        sums = lens.render_layers(img0, alpha0, z, spp=8, dp=None, wvln=WVLN, scales=scales, pupil_points=(x2[:8], y2[:8]),
                                  return_sums=True)
        hand, _ = hand_depth(lens, img0, alpha0, z, scales, x2[:8], y2[:8], G[:1], sums[2], None, WVLN)
        assert torch.equal(one, sums[0]) and torch.equal(zt.grad, hand[:, 0])
        # depth_grad=False, and depth_grad=True under no_grad or without a tensor that requires one: the plain call
        kw = dict(spp=8, dp=DP, wvln=WVLN, pupil_points=(x2[:8], y2[:8]))
        ref = lens.render_layers(img0, alpha0, z, scales=scales, **kw)
        zt, st = leaves()
        off = lens.render_layers(img0, alpha0, zt, scales=st, **kw)
        with torch.no_grad():
            quiet = lens.render_layers(img0, alpha0, zt, scales=st, depth_grad=True, **kw)
        on = lens.render_layers(img0, alpha0, z, scales=scales, depth_grad=True, **kw)
        sums = lens.render_layers(img0, alpha0, zt, scales=st, return_sums=True, **kw)
        for other in (off, quiet, on, sums[:2]):
            assert all(torch.equal(a, b) and a.grad_fn is None for a, b in zip(other, ref))
        with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
            lens.render_layers(img0, alpha0, zt, scales=st, depth_grad=True, return_sums=True, **kw)


def test_depth_grad_composes_with_scene_grad_and_dp_grad(lens):
    """One backward runs the three kernels from the one record.  The depths, the scales and h, f, w get what each option
    alone gives them, bit for bit (fixed summation orders); img and alpha are held to §7q's two-run bound, since that
    kernel's atomics give no two runs the same bits."""
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        L, Ht, Wt = 3, 5, 9
        z = list(DEPTHS3)
        scales = [half_cover_scale(lens, d, lens.focus_depth) for d in z]
        alpha0 = mixed_alpha(L, Ht, Wt, seed=61)
        img0 = texture(L * 3, Ht, Wt, seed=62).view(L, 3, Ht, Wt)
        G = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(65)).to(DEV)
        x2, y2 = pupil_points(lens, 8, seed=66)
        kw = dict(spp=8, wvln=WVLN, pupil_points=(x2, y2))

        def run(scene, dpg, zg):
            img, alpha = img0.clone().requires_grad_(), alpha0.clone().requires_grad_()
            hfw = [torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=True) for v in DP[:3]]
            zt = torch.tensor(z, dtype=torch.float64, device=DEV, requires_grad=True)
            st = torch.tensor(scales, dtype=torch.float64, device=DEV, requires_grad=True)
            vs = lens.render_layers(img, alpha, zt, dp=(*hfw, DP[3]), scales=st, scene_grad=scene, dp_grad=dpg,
                                    depth_grad=zg, **kw)
            sum((v * G[n]).sum() for n, v in enumerate(vs)).backward()
            return img.grad, alpha.grad, [v.grad for v in hfw], zt.grad, st.grad, vs

        every = run(True, True, True)
        alone = run(False, False, True)
        others = run(True, True, False)
        for a, b, c in zip(every[5], alone[5], others[5]):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.equal(every[3], alone[3]) and torch.equal(every[4], alone[4]) and bool((every[3] != 0).all())
        assert others[3] is None and others[4] is None
        assert alone[0] is None and alone[1] is None and all(g is None for g in alone[2])
        assert all(torch.equal(a, b) for a, b in zip(every[2], others[2])) and all(bool(a != 0) for a in every[2])
        den = lens.render_layers(img0, alpha0, z, dp=DP, scales=scales, return_sums=True, **kw)[3]
        ha, ht, ba, bt = hand_grads(lens, img0, alpha0, z, scales, x2, y2, G, den, DP, WVLN)
        assert_fp32_of("composed, img", every[0], ht, bt)
        assert_fp32_of("composed, alpha", every[1], ha, ba)


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
        kw = dict(spp=8, wvln=WVLN, pupil_points=(x2, y2), dp=DP)
        G = torch.randn(2, 2, 3, H, W, generator=torch.Generator().manual_seed(73)).to(DEV)
        zt = torch.tensor(zs, dtype=torch.float64, device=DEV, requires_grad=True)
        gL, gR = lens.render_rgbd(frame, depth, layer_depths=zt, scales=scales, depth_grad=True, **kw)
        pL, pR = lens.render_rgbd(frame, depth, layer_depths=zs, scales=scales, **kw)
        assert torch.equal(gL, pL) and torch.equal(gR, pR) and gL.grad_fn is not None and pL.grad_fn is None
        ((gL * G[0]).sum() + (gR * G[1]).sum()).backward()
        per_frame = []
        for b in range(2):
            alpha = layers_from_rgbd(depth[b, 0], zs)
            sums = lens.render_layers(frame[b], alpha, zs, scales=scales, return_sums=True, **kw)
            per_frame.append(hand_depth(lens, frame[b].contiguous(), alpha, zs, scales, x2, y2, G[:, b], sums[3], DP, WVLN)[0][:, 0])
        print(f"render_rgbd: {zt.grad.tolist()} = {per_frame[0].tolist()} + {per_frame[1].tolist()}")
        assert torch.equal(zt.grad, per_frame[0] + per_frame[1]) and bool((per_frame[0] != 0).any())
        # depths made of the map take none
        auto = lens.render_rgbd(frame, depth.clone().requires_grad_(), n_layers=2, depth_grad=True, **kw)
        assert auto[0].grad_fn is None


# ------------------------------------------------------------------------------------ 8. kernel against kernel
BAND = 2.0 ** -6


def off_the_boundaries(lens, alpha, tex, z, inv, layer, spp, seed):
    """Pupil points none of whose live rays lands within BAND of a texel boundary on `layer`: rays that do are given
    the pupil point of the next draw, until none is left -> x2, y2, the forward's output with its landing record."""
    Ht, Wt = (int(v) for v in tex.shape[-2:])
    x2, y2 = pupil_points(lens, spp, seed=seed)
    for n in range(1, 40):
        out = layer_batch(lens, alpha, tex, z, inv, x2, y2, DP, WVLN, landing=True)
        land = out["landing"].cpu().numpy()
        live = land[0] != 0
        _, _, fu, fv = tap_origin(np.where(live, land[3 + 2 * layer], 0), np.where(live, land[4 + 2 * layer], 0), inv[layer], Ht, Wt)
        bad = live & ((fu < BAND) | (fu > 1 - BAND) | (fv < BAND) | (fv > 1 - BAND))
        if not bad.any():
            return x2, y2, out
        nx, ny = pupil_points(lens, spp, seed=seed + 100 * n)
        bad = torch.from_numpy(bad).to(DEV)
        x2, y2 = torch.where(bad, nx, x2).contiguous(), torch.where(bad, ny, y2).contiguous()
    raise AssertionError("rays are still flagged after 39 draws")


@pytest.mark.parametrize("scene", ["occlusion", "ramp"])
def test_a_central_difference_through_the_forward_kernel_in_one_depth(lens, scene):
    """F(z) = <gnum, num(z)> of the FORWARD kernel at z_l +- h against the backward's gdepth_l (den and ra do not depend
    on z).  Rays within BAND = 2^-6 of a texel boundary on layer l are drawn again first (none is left: asserted), and
    h, a power of two so that z_l +- h are fp32 numbers, moves no ray's u or v by more than BAND / 2: every ray stays in
    its bilinear cell, where F is a polynomial in z whose third-order term is below 10^-4 of the first at this step.
    What remains is the forward's fp32 rounding: it forms u from an fp32 landing, a product, a difference and u - 0.5,
    at most 4 half-spacings of the largest |u| a ray reaches, at both ends of the difference: the rounding term
    (4 * 2^-24 * Umax / h) sum_rays (|Pu| + |Pv|), with Pu, Pv of the restatement on the forward's record.  Printed next
    to the gradient; where the gradient exceeds the term, the sign and agreement within twice the term are asserted.
    No other bound is asserted.  occlusion: §7p's test 5, an opaque half-plane at -700 mm before an opaque background
    at -3000 mm, moved layer 0.  ramp: one opaque layer whose texture is linear in the column: the forward is linear
    in z up to that rounding."""
    spp = 8
    with sensor(lens, **SMALL):
        H, W = lens.sensor_res
        Ht, Wt = H, W
        if scene == "occlusion":
            z = [-700.0, -3000.0]
            alpha = torch.zeros(2, Ht, Wt, device=DEV)
            alpha[0, :, Wt // 2:] = 1.0
            alpha[1] = 1.0
            tex = torch.zeros(2, 2, Ht, Wt, device=DEV)
            tex[0, 0], tex[1, 1] = 1.0, 1.0
        else:
            z = [-700.0]
            alpha = torch.ones(1, Ht, Wt, device=DEV)
            cols = torch.arange(Wt, dtype=torch.float32, device=DEV)
            tex = torch.stack((0.25 * cols, 4.0 - 0.125 * cols))[None, :, None, :].expand(1, 2, Ht, Wt).contiguous()
        layer = 0
        scales = [magnification(lens, d, lens.focus_depth) for d in z]
        inv = [inv_texel_of(lens, s, Wt) for s in scales]
        x2, y2, out = off_the_boundaries(lens, alpha, tex, z, inv, layer, spp, seed=51)
        # G = +1 on L and -1 on R, with the other signs on the second plane: the loss is a disparity, to which the rays of
        # the two pupil halves add with one sign (a random G cancels to below the rounding term), and the two planes --
        # foreground and background, or ramps of opposite slope -- move against each other
        G = torch.ones(2, 2, H, W, dtype=torch.float64, device=DEV)
        G[1, 0], G[0, 1] = -1.0, -1.0
        gnum = gnum_from_image_grad(G, out["den"]).contiguous()
        grad, rd = layer_depth_grad_batch(lens, alpha, tex, z, inv, x2, y2, out["trips"], gnum, DP, WVLN, ray_dir=True)
        ref = reference(out["landing"], rd, len(z), 2, alpha, tex, inv, gnum)
        assert_grad(scene, grad, ref, len(z))
        live = out["landing"][0].cpu().numpy() != 0
        d = rd.cpu().numpy().astype(np.float64)
        inv32 = float(np.float32(inv[layer]))
        slope = inv32 * max(float(np.abs(d[0] / d[2])[live].max()), float(np.abs(d[1] / d[2])[live].max()))
        h = 2.0 ** np.floor(np.log2(BAND / 2 / slope))
        assert h * slope <= BAND / 2 and float(np.float32(z[layer] + h)) - z[layer] == h == z[layer] - float(np.float32(z[layer] - h))

        def F(zl):
            zz = list(z)
            zz[layer] = zl
            o = layer_batch(lens, alpha, tex, zz, inv, x2, y2, DP, WVLN)
            assert torch.equal(o["den"], out["den"])
            return float((gnum * o["num"]).sum())

        cd = (F(z[layer] + h) - F(z[layer] - h)) / (2 * h)
        Umax = 2.0 ** np.ceil(np.log2(float(max(Ht, Wt)) * 2))
        term = 4 * 2.0 ** -24 * Umax / h * float((np.abs(ref["Pu"][layer]) + np.abs(ref["Pv"][layer]))[live].sum())
        g = float(grad[layer, 0])
        print(f"{scene}: d<gnum, num>/dz_{layer}: backward {g:+.6e}, central difference {cd:+.6e}, difference {cd - g:+.3e}, "
              f"rounding term {term:.3e}, h {h} mm ({h * slope:.2e} texels at most)")
        assert np.isfinite(cd) and g != 0
        if abs(g) > term:
            assert np.sign(cd) == np.sign(g) and abs(cd - g) <= 2 * term, (cd, g, term)
        if scene == "ramp":
            # gz = sum q (-inv sx) slope on the rays inside the texture, whichever cell they land in
            land = out["landing"].cpu().numpy()
            c0, _, _, _ = tap_origin(np.where(live, land[3], 0), np.where(live, land[4], 0), inv[0], Ht, Wt)
            inside = live & (c0 >= 0) & (c0 < Wt - 1)
            wr = np.where(live, land[1:3].astype(np.float64) * land[0].astype(np.float64), 0.0)
            gn = gnum.cpu().numpy()
            q = wr[0] * gn[0][:, None] + wr[1] * gn[1][:, None]
            terms = np.where(inside, inv32 * -((q[0] * 0.25 + q[1] * -0.125) * (d[0] / d[2])), 0.0)
            assert 0.2 < inside[live].mean() and abs(g - terms.sum()) <= 2 * (inside.sum() + 8) * 2.0 ** -53 * np.abs(terms).sum()
            assert (ref["Pu"][0][live & ~inside] == 0).all()


# ------------------------------------------------------------------------------------ 9. physics
def test_the_disparity_s_depth_gradient_changes_sign_across_focus(lens):
    """A vertical edge on one opaque plane, the lens focused at -1000 mm.  J = sum (L - R) G with G = sign(L - R), the
    sign of the disparity, is the summed |L - R|: 0 in focus and growing with defocus on either side.  Moving a plane in
    front of focus (-600 mm) towards the lens (z up) defocuses it further, dJ/dz > 0; moving a plane behind focus
    (-2500 mm) towards the lens brings it nearer to focus, dJ/dz < 0.  The texture keeps its extent (scale is a
    constant), and the edge sits on the axis, so it does not move."""
    spp = 8
    with sensor(lens, **SMALL):
        H, W = lens.sensor_res
        tex = torch.zeros(1, 1, H, W, device=DEV)
        tex[..., W // 2:] = 1.0
        x2, y2 = pupil_points(lens, spp, seed=91)
        got = {}
        for depth in (-600.0, -2500.0):
            scale = magnification(lens, depth, lens.focus_depth)
            kw = dict(spp=spp, dp=DP, wvln=WVLN, scale=scale, pupil_points=(x2, y2))
            pL, pR = lens.render_plane(tex, depth, **kw)
            Gs = torch.sign(pL - pR)
            zt = torch.tensor(depth, dtype=torch.float64, requires_grad=True)
            vL, vR = lens.render_plane(tex, zt, depth_grad=True, **kw)
            ((vL - vR) * Gs).sum().backward()
            got[depth] = float(zt.grad)
            print(f"depth {depth}: J = sum|L - R| = {float(((pL - pR) * Gs).sum()):.4f}, dJ/dz = {got[depth]:+.6e}")
            assert float((Gs != 0).float().mean()) > 0.02
        assert got[-600.0] > 0 > got[-2500.0], got
