"""k_render_layers_grad (csrc/sdirt_render_rt.hip) on the GPU: the layered render's backward, a float64
scatter into the textures and the coverage maps.

  1. the kernel against tests/render_layers_grad_f64.py (numpy, written from the text of §7q) on the forward's own
     landing record, within 2 (n + 5 L + 22) 2^-53 sum|term| per texel;
  2. all 24 instantiations;
  3. kernel against kernel: <gnum, num(tex')> = <gtex, tex'>, and the forward's exact difference in eight alpha texels;
  4. occlusion: hidden background texels get exactly nothing, the sign of a foreground texel's coverage gradient;
  5. L = 1 with a null alpha, alpha == 1, and render_plane(scene_grad=True);
  6. the autograd surface of render_layers and render_rgbd;
  7. the C entry directly: it accumulates, null outputs, guard bands, refusals, a side stream, two runs.

Float64 atomic sums depend on arrival order: nothing the kernel adds up is asserted bit-equal.  Sensors, textures and
the seeded alpha stacks are those of test_gpu_render_layers.py and test_gpu_render_raytraced_edges.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_layers_grad_f64 as RG
from test_gpu_render_layers import (CASES_3, DEPTHS3, alpha_stack, land_points, layer_inv_texels, lens, rays,  # noqa: F401
                                    stack_depths)
from test_gpu_render_raytraced import DP, DP_BIG, DEV, SMALL, WIDE, WVLN, pupil_points, sensor
from test_gpu_render_raytraced_edges import RAGGED, _guarded, half_cover_scale, inv_texel_of, magnification, texture

from sdirt_amd import _lib
from sdirt_amd.basics import WAVE_RGB, dptr, stream_ptr
from sdirt_amd.render_rt import (gnum_from_image_grad, layer_batch, layer_grad_batch, layers_from_rgbd, sensor_axes)

pytestmark = pytest.mark.gpu
FLOOR = 0.05
U = 2.0 ** -53


def seeded_gnum(V, T, H, W, seed):
    """Normal float64 of both signs."""
    return torch.randn(V, T, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(DEV)


def reference(land, L, V, alpha, tex, inv, gnum):
    """The numpy restatement on a launch's landing record."""
    lx, ly = land_points(land, L)
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return RG.layer_grads_f64(cpu(lx), cpu(ly), cpu(land[0]), cpu(land[1:1 + V]), cpu(alpha), cpu(tex), inv, cpu(gnum))


def assert_grads(tag, galpha, gtex, ref, L, times=1):
    """Kernel buffers against `times` x the restatement, within `times` x the bound of §7q, texel by texel."""
    for name, g in (("alpha", galpha), ("tex", gtex)):
        if g is None:
            continue
        want, ab = ref["g" + name], ref["abs_" + name]
        bound = times * RG.bound(ref["n_" + name], L, ab)
        got = g.cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.abs(got - times * want)
        print(f"{tag}: g{name} worst |kernel - f64| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
              f"most terms in a texel {int(ref['n_' + name].max())}")
        assert (err <= bound).all()
        assert (ab > 0).any() and np.abs(want).max() > 0


def forward_and_grads(lens, alpha, tex, depths, inv, r, dp, gnum, **kw):
    out = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], dp, WVLN, landing=True)
    ga, gt = layer_grad_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], out["trips"], gnum, dp, WVLN, **kw)
    return out, ga, gt


def stopped_with_something_behind(ref, ra):
    """Share of the live rays that an opaque texel stops (T_l != 0, a_l == 1) in front of a layer they would read
    coverage from (a_m != 0 for some m > l): the rays whose gradient needs R_{l+1}, which the forward never formed."""
    a, Tb = ref["a"], ref["T_before"]
    live = ra.cpu().numpy() != 0
    stops = (Tb != 0) & (a == 1)
    behind = np.flip(np.cumsum(np.flip(a != 0, 0), 0), 0) - (a != 0)       # covered layers strictly behind l
    return float(((stops & (behind > 0)).any(0))[live].mean())


# ------------------------------------------------------------------------------------ 1. against the restatement
TINY = [(3, (1, 1), 8, False, 2, 0.5), (2, (1, 7), 5, True, 3, 0.5), (3, (7, 1), 8, False, 1, 0.5)]


@pytest.mark.parametrize("L, shape, spp, shared, planes, back", CASES_3 + TINY)
def test_gradients_equal_the_numpy_restatement(lens, rays, L, shape, spp, shared, planes, back):
    Ht, Wt = shape
    depths = stack_depths(L)
    r = rays(spp, depths)
    tag = f"L {L}, {Ht} x {Wt}, spp {spp}, {'shared' if shared else 'per-layer'}, {planes} planes"
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        assert len(set(np.float32(inv).tolist())) == L           # another texel size on every layer
        alpha = alpha_stack(L, Ht, Wt, back=back)
        if min(Ht, Wt) == 1:                                     # both taps on one texel: fractional coverage as well
            alpha = alpha * torch.rand(L, Ht, Wt, generator=torch.Generator().manual_seed(5)).to(DEV).clamp_min(0.25)
            alpha[-1] = 1.0
        tex = texture(planes, Ht, Wt, seed=31) if shared else texture(L * planes, Ht, Wt, seed=32).view(L, planes, Ht, Wt)
        gnum = seeded_gnum(2, planes, H, W, seed=33)
        assert bool((gnum > 0).any()) and bool((gnum < 0).any())
        out, ga, gt = forward_and_grads(lens, alpha, tex, depths, inv, r, DP, gnum)
        assert ga.shape == alpha.shape and gt.shape == tex.shape and ga.dtype == gt.dtype == torch.float64
        ref = reference(out["landing"], L, 2, alpha, tex, inv, gnum)
        if L > 1 and min(Ht, Wt) > 1:                            # the seeded binary stacks of test_gpu_render_layers.py
            share = stopped_with_something_behind(ref, out["landing"][0])
            print(f"{tag}: {share:.3f} of the live rays stop at an opaque texel with coverage behind it")
            assert share >= FLOOR, share
        assert_grads(tag, ga, gt, ref, L)


# ------------------------------------------------------------------------------------ 2. every instantiation
@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("dp", [None, DP, DP_BIG], ids=["none", "small", "big"])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_gradients_of_every_instantiation(lens, rays, precision, dp, planes):
    """k_render_layers_grad<M, DP, NT>: 2 x 3 x 4, at L = 2, each against the landing record of its own forward."""
    spp, Ht, Wt, L = 8, 7, 12, 2
    depths = stack_depths(L)
    r = rays(spp, depths)
    V = 1 if dp is None else 2
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, seed=41)
        tex = texture(L * 4, Ht, Wt, seed=42).view(L, 4, Ht, Wt)[:, :planes].contiguous()
        gnum = seeded_gnum(V, planes, H, W, seed=43)
        out, ga, gt = forward_and_grads(lens, alpha, tex, depths, inv, r, dp, gnum)
        ref = reference(out["landing"], L, V, alpha, tex, inv, gnum)
        assert_grads(f"{precision}, dp {dp}, {planes} planes", ga, gt, ref, L)


# ------------------------------------------------------------------------------------ 3. kernel against kernel
def _dot(lens, alpha, tex, depths, inv, r, gnum):
    """<gnum, num> of the forward kernel and the same with every factor's absolute value (all its terms >= 0)."""
    num = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN)["num"]
    numabs = layer_batch(lens, alpha, tex.abs(), depths, inv, r["x2"], r["y2"], DP, WVLN)["num"]
    return float((gnum * num).sum()), float((gnum.abs() * numabs).sum())


@pytest.mark.parametrize("L, shape, spp, shared", [(3, (5, 141), 8, False), (16, (2, 3), 5, True), (2, (11, 280), 8, True)])
def test_the_dot_product_identity_and_exact_differences_in_alpha(lens, rays, L, shape, spp, shared):
    """Forward and backward kernel against each other.  The forward's <gnum, num> carries, per elementary product, at
    most 7 (lookup) + 3 L (g, T, c) + 3 (wr, the term) + S (the sum over s) + 1 roundings and log2 P more from torch's
    sum of the P = V T H W products: 2 (3 L + S + 11 + log2 P) 2^-53 of the same dot product on absolute values.  The
    backward's side carries §7q's bound per texel (times |tex'|) and the rounding of its own dot product."""
    Ht, Wt = shape
    depths = stack_depths(L)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, seed=51)
        tshape = (3, Ht, Wt) if shared else (L, 3, Ht, Wt)
        tex = texture(int(np.prod(tshape[:-2])), Ht, Wt, seed=52).view(tshape)
        other = texture(int(np.prod(tshape[:-2])), Ht, Wt, seed=53).view(tshape)
        gnum = seeded_gnum(2, 3, H, W, seed=54)
        out, ga, gt = forward_and_grads(lens, alpha, tex, depths, inv, r, DP, gnum)
        ref = reference(out["landing"], L, 2, alpha, tex, inv, gnum)
        eps_f = 2 * (3 * L + spp + 11 + np.log2(gnum.numel())) * U
        # colour: num is linear in tex and gtex does not depend on it
        lhs, lhs_abs = _dot(lens, alpha, other, depths, inv, r, gnum)
        o64 = other.double()
        rhs = float((gt * o64).sum())
        rhs_abs = torch.from_numpy(ref["abs_tex"]).to(DEV) * o64.abs()
        tol = eps_f * lhs_abs + float((torch.from_numpy(RG.bound(ref["n_tex"], L, ref["abs_tex"])).to(DEV) * o64.abs()).sum()) \
            + 2 * np.log2(o64.numel()) * U * float(rhs_abs.sum())
        print(f"L {L}, {Ht} x {Wt}: <gnum, num(tex')> {lhs:.12e}, <gtex, tex'> {rhs:.12e}, |difference| / tolerance "
              f"{abs(lhs - rhs) / tol:.3f}")
        assert abs(lhs - rhs) <= tol and abs(lhs) > 1e3 * tol
        # coverage: <gnum, num> is affine in one texel of alpha -- eight texels that rays read, spread over the stack
        read = np.flatnonzero(ref["n_alpha"].reshape(-1) > 0)
        picks = read[np.linspace(0, len(read) - 1, 8).astype(int)]
        assert len(set(picks.tolist())) == 8
        for flat in picks:
            pos = np.unravel_index(flat, ref["n_alpha"].shape)
            F = []
            for v in (1.0, 0.0):
                a = alpha.clone()
                a[pos] = v
                F.append(_dot(lens, a, tex, depths, inv, r, gnum))
            tol = eps_f * (F[0][1] + F[1][1]) + float(RG.bound(ref["n_alpha"][pos], L, ref["abs_alpha"][pos]))
            err = abs((F[0][0] - F[1][0]) - float(ga[pos]))
            print(f"  alpha{pos}: difference {F[0][0] - F[1][0]:+.9e}, galpha {float(ga[pos]):+.9e}, / tolerance {err / tol:.3f}")
            assert err <= tol, (pos, err, tol)


# ------------------------------------------------------------------------------------ 4. occlusion
@pytest.mark.parametrize("bright", [False, True], ids=["dark-background", "bright-background"])
def test_hidden_texels_get_nothing_and_the_matte_s_gradient_has_the_sign_of_the_contrast(lens, bright):
    """§7p's half-plane scene: an opaque foreground (colour 0.5) at -700 mm over an opaque background (colour B) at
    -3000 mm, gnum == 1.  For a ray the foreground stops, e_0 = D_0 - R_1 = q 0.5 - q B."""
    z = [-700.0, -3000.0]
    spp, B = 8, (1.0 if bright else 0.0)
    with sensor(lens, **SMALL):
        H, W = lens.sensor_res
        Ht, Wt = H, W
        inv = [inv_texel_of(lens, magnification(lens, d, lens.focus_depth), Wt) for d in z]
        alpha = torch.zeros(2, Ht, Wt, device=DEV)
        alpha[0, :, Wt // 2:] = 1.0
        alpha[1] = 1.0
        tex = torch.stack((torch.full((1, Ht, Wt), 0.5), torch.full((1, Ht, Wt), B))).to(DEV)
        x2, y2 = pupil_points(lens, spp, seed=51)
        gnum = torch.ones(2, 1, H, W, dtype=torch.float64, device=DEV)
        out, ga, gt = forward_and_grads(lens, alpha, tex, z, inv, dict(x2=x2, y2=y2), DP, gnum)
        land = out["landing"]
        ref = reference(land, 2, 2, alpha, tex, inv, gnum)
        assert_grads(f"B {B}", ga, gt, ref, 2)
        # background texels that rays land on, but only rays the foreground has stopped
        live = land[0].cpu().numpy() != 0
        idx, w = RG.taps(np.where(live, land[5].cpu().numpy(), 0), np.where(live, land[6].cpu().numpy(), 0), inv[1], Ht, Wt)
        touched = np.zeros(Ht * Wt, np.int64)
        for j in range(4):
            np.add.at(touched, idx[j][live], 1)
        hidden = torch.from_numpy((touched.reshape(Ht, Wt) > 0) & (ref["n_tex"][1, 0] == 0)).to(DEV)
        print(f"{int(hidden.sum())} of {Ht * Wt} background texels are reached only behind the foreground")
        assert int(hidden.sum()) > 0.1 * Ht * Wt
        assert bool((gt[1, 0][hidden] == 0).all()) and bool((ga[1][hidden] == 0).all())
        assert bool((gt[1, 0][~hidden] != 0).any())
        # an interior foreground texel
        pos = (Ht // 2, 3 * Wt // 4)
        a, Tb = ref["a"], ref["T_before"]
        idx0, w0 = RG.taps(np.where(live, land[3].cpu().numpy(), 0), np.where(live, land[4].cpu().numpy(), 0), inv[0], Ht, Wt)
        want, n = 0.0, 0
        for j in range(4):
            sel = live & (idx0[j] == pos[0] * Wt + pos[1])
            assert (a[0][sel] == 1).all() and (a[1][sel] == 1).all()
            want -= float(((ref["q"][0] * (B - 0.5)) * w0[j])[sel].sum())
            n += int(sel.sum())
        got = float(ga[0][pos])
        bound = float(RG.bound(n, 2, ref["abs_alpha"][0][pos]))
        print(f"galpha at the foreground texel {pos}: {got:+.6e} from {n} terms, -sum q (B - t_fg) w_j {want:+.6e}")
        assert n > 0 and abs(got - want) <= bound
        assert (got < 0) if bright else (got > 0)


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
        out, ga, gt = forward_and_grads(lens, ones, tex, [depth], inv, r, DP, gnum)
        ref = reference(out["landing"], 1, 2, ones, tex, inv, gnum)
        assert_grads("alpha == 1", ga, gt, ref, 1)
        # ... where e_0 = D_0: the restatement's sum of q_k t_k w_j
        idx, w = RG.taps(np.where(out["landing"][0].cpu().numpy() != 0, out["landing"][3].cpu().numpy(), 0),
                         np.where(out["landing"][0].cpu().numpy() != 0, out["landing"][4].cpu().numpy(), 0), inv[0], Ht, Wt)
        live = out["landing"][0].cpu().numpy() != 0
        direct = np.zeros(Ht * Wt)
        for j in range(4):
            np.add.at(direct, idx[j][live], (ref["D"][0] * w[j])[live])
        assert (np.abs(ga[0].cpu().numpy().reshape(-1) - direct) <= RG.bound(ref["n_alpha"][0], 1, ref["abs_alpha"][0]).reshape(-1)).all()
        na, nt = layer_grad_batch(lens, None, tex, [depth], inv, r["x2"], r["y2"], out["trips"], gnum, DP, WVLN)
        assert na is None
        assert_grads("null alpha", None, nt, ref, 1)
        # render_plane(scene_grad=True): img [1, C, Ht, Wt], the loss sum_v <G_v, view_v>
        img = tex[None].clone().requires_grad_()
        G = torch.randn(2, 1, planes, H, W, generator=torch.Generator().manual_seed(63)).to(DEV)
        vL, vR = lens.render_plane(img, depth, spp=spp, dp=DP, wvln=WVLN, scale=scale, pupil_points=(r["x2"], r["y2"]),
                                   scene_grad=True)
        plain = lens.render_plane(tex[None], depth, spp=spp, dp=DP, wvln=WVLN, scale=scale, pupil_points=(r["x2"], r["y2"]),
                                  return_sums=True)
        assert torch.equal(vL, plain[0]) and torch.equal(vR, plain[1]) and vL.grad_fn is not None
        ((vL * G[0]).sum() + (vR * G[1]).sum()).backward()
        assert img.grad.shape == img.shape and img.grad.dtype == torch.float32
        gn = gnum_from_image_grad(G[:, 0], plain[3])
        _, hand = layer_grad_batch(lens, None, tex, [depth], inv, r["x2"], r["y2"], out["trips"], gn, DP, WVLN)
        ref = reference(out["landing"], 1, 2, None, tex, inv, gn)
        assert_fp32_of("render_plane, img", img.grad[0], hand, torch.from_numpy(RG.bound(ref["n_tex"], 1, ref["abs_tex"])).to(DEV))


# ------------------------------------------------------------------------------------ 6. the autograd surface
def hand_grads(lens, img, alpha, z, scales, x2, y2, G, den, dp, wvln, photometric=False):
    """render_layers' gradients by hand for one wavelength: gnum = G / den_total, then layer_grad_batch over the chunks
    of 64 samples into one pair of buffers.  -> galpha, gimg float64, and the restatement's bounds of both (summed
    over the chunks, which are added into the same texels)."""
    H, W = lens.sensor_res
    L, (Ht, Wt) = alpha.shape[0], alpha.shape[-2:]
    V = 1 if dp is None else 2
    inv = [inv_texel_of(lens, s, Wt) for s in scales]
    gnum = gnum_from_image_grad(G, den, x2.shape[0], photometric)
    ga = torch.zeros(alpha.shape, dtype=torch.float64, device=DEV)
    gt = torch.zeros(img.shape, dtype=torch.float64, device=DEV)
    ba, bt = np.zeros(alpha.shape), np.zeros(img.shape)
    for s0 in range(0, x2.shape[0], 64):
        xs, ys = x2[s0:s0 + 64], y2[s0:s0 + 64]
        out = layer_batch(lens, alpha, img, z, inv, xs, ys, dp, wvln, landing=True)
        layer_grad_batch(lens, alpha, img, z, inv, xs, ys, out["trips"], gnum, dp, wvln, galpha=ga, gtex=gt)
        ref = reference(out["landing"], L, V, alpha, img, inv, gnum)
        ba += RG.bound(ref["n_alpha"], L, ref["abs_alpha"])
        bt += RG.bound(ref["n_tex"], L, ref["abs_tex"])
    return ga, gt, torch.from_numpy(ba).to(DEV), torch.from_numpy(bt).to(DEV)


def assert_fp32_of(tag, grad, hand, bound):
    """An fp32 gradient against the float64 buffers of a second run: two arrival orders and one rounding to fp32."""
    assert grad is not None and grad.dtype == torch.float32 and grad.shape == hand.shape, tag
    tol = 2 * bound + 2.0 ** -24 * hand.abs()
    err = (grad.double() - hand).abs()
    print(f"{tag}: worst |autograd - by hand| / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all()) and float(hand.abs().max()) > 0, tag


def test_render_layers_backward_is_the_entry_run_by_hand(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        L, Ht, Wt = 3, 5, 9
        z = list(DEPTHS3)
        scales = [half_cover_scale(lens, d, lens.focus_depth) for d in z]
        alpha0 = alpha_stack(L, Ht, Wt, seed=61)
        img0 = texture(L * 3, Ht, Wt, seed=62).view(L, 3, Ht, Wt)
        gen = torch.Generator().manual_seed(64)
        G = torch.randn(2, 3, H, W, generator=gen).to(DEV)
        x2, y2 = pupil_points(lens, 128, seed=63)

        def run(img_src, spp, dp=DP, wvln=WVLN, pts=None, **kw):
            img, alpha = img_src.clone().requires_grad_(), alpha0.clone().requires_grad_()
            pts = (x2[:spp], y2[:spp]) if pts is None else pts
            views = lens.render_layers(img, alpha, z, spp=spp, dp=dp, wvln=wvln, scales=scales, pupil_points=pts,
                                       scene_grad=True, **kw)
            plain = lens.render_layers(img_src, alpha0, z, spp=spp, dp=dp, wvln=wvln, scales=scales, pupil_points=pts,
                                       return_sums=True, **kw)
            views = views if isinstance(views, tuple) else (views,)
            for v, p in zip(views, plain):
                assert torch.equal(v, p) and v.grad_fn is not None and p.grad_fn is None
            sum((v * G[n]).sum() for n, v in enumerate(views)).backward()
            assert img.grad.shape == img.shape and alpha.grad.shape == alpha.shape
            return img.grad, alpha.grad, plain[len(views) + 1]          # den

        # 128 samples: two chunks, both divided by the TOTAL den
        gi, ga, den = run(img0, 128)
        ha, ht, ba, bt = hand_grads(lens, img0, alpha0, z, scales, x2, y2, G, den, DP, WVLN)
        assert_fp32_of("128 spp, img", gi, ht, bt)
        assert_fp32_of("128 spp, alpha", ga, ha, ba)
        # photometric, no dual pixel, a shared image
        gi, ga, den = run(img0, 8, photometric=True)
        ha, ht, ba, bt = hand_grads(lens, img0, alpha0, z, scales, x2[:8], y2[:8], G, den, DP, WVLN, photometric=True)
        assert_fp32_of("photometric, img", gi, ht, bt)
        assert_fp32_of("photometric, alpha", ga, ha, ba)
        gi, ga, den = run(img0[1], 8, dp=None)
        ha, ht, ba, bt = hand_grads(lens, img0[1], alpha0, z, scales, x2[:8], y2[:8], G[:1], den, None, WVLN)
        assert_fp32_of("dp=None, shared img", gi, ht, bt)
        assert_fp32_of("dp=None, alpha", ga, ha, ba)
        # per-channel wavelengths: every channel through its own trace, alpha summed over the channels
        xs, ys = zip(*(pupil_points(lens, 8, seed=64 + c) for c in range(3)))
        x3, y3 = torch.stack(xs), torch.stack(ys)
        for src in (img0, img0[1]):
            gi, ga, den = run(src, 8, wvln=WAVE_RGB, pts=(x3, y3))
            assert den.shape == (2, 3, H, W)
            sa, sba = 0, 0
            for c in range(3):
                ch = (src[:, c:c + 1] if src.dim() == 4 else src[c:c + 1]).contiguous()
                ha, ht, ba, bt = hand_grads(lens, ch, alpha0, z, scales, x3[c], y3[c], G[:, c:c + 1], den[:, c], DP, WAVE_RGB[c])
                assert_fp32_of(f"wavelength {c}, img", (gi[:, c:c + 1] if src.dim() == 4 else gi[c:c + 1]).contiguous(), ht, bt)
                sa, sba = sa + ha, sba + ba
            assert_fp32_of("three wavelengths, alpha", ga, sa, sba)
        # only one of the two asks for a gradient
        img = img0.clone().requires_grad_()
        vL, _ = lens.render_layers(img, alpha0, z, spp=8, dp=DP, wvln=WVLN, scales=scales, pupil_points=(x2[:8], y2[:8]),
                                   scene_grad=True)
        vL.sum().backward()
        assert img.grad is not None and alpha0.grad is None
        # scene_grad=False, and scene_grad=True under no_grad: the plain call, no grad_fn
        img, alpha = img0.clone().requires_grad_(), alpha0.clone().requires_grad_()
        kw = dict(spp=8, dp=DP, wvln=WVLN, scales=scales, pupil_points=(x2[:8], y2[:8]))
        ref = lens.render_layers(img0, alpha0, z, **kw)
        off = lens.render_layers(img, alpha, z, **kw)
        with torch.no_grad():
            quiet = lens.render_layers(img, alpha, z, scene_grad=True, **kw)
        on = lens.render_layers(img0, alpha0, z, scene_grad=True, return_sums=True, **kw)        # nothing requires one
        for other in (off, quiet, on[:2]):
            assert all(torch.equal(a, b) and a.grad_fn is None for a, b in zip(other, ref))
        with pytest.raises(ValueError, match="return_sums with a recorded gradient"):
            lens.render_layers(img, alpha, z, scene_grad=True, return_sums=True, **kw)


def test_render_rgbd_backward_sums_the_shared_image_s_layers_and_gives_depth_nothing(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        frame0 = texture(2 * 3, H, W, seed=71).view(2, 3, H, W)
        x2, y2 = pupil_points(lens, 8, seed=72)
        depth = torch.full((2, 1, H, W), -3000.0, device=DEV)
        depth[0, 0, :, 20:40] = -700.0
        depth[1, 0, 1:, 5:30] = -700.0
        zs = [-700.0, -3000.0]
        scales = [magnification(lens, d, lens.focus_depth) for d in zs]
        kw = dict(spp=8, dp=DP, wvln=WVLN, pupil_points=(x2, y2))
        G = torch.randn(2, 2, 3, H, W, generator=torch.Generator().manual_seed(73)).to(DEV)
        frame, dleaf = frame0.clone().requires_grad_(), depth.clone().requires_grad_()
        gL, gR = lens.render_rgbd(frame, dleaf, layer_depths=zs, scales=scales, scene_grad=True, **kw)
        pL, pR = lens.render_rgbd(frame, dleaf, layer_depths=zs, scales=scales, **kw)
        assert torch.equal(gL, pL) and torch.equal(gR, pR) and gL.grad_fn is not None and pL.grad_fn is None
        ((gL * G[0]).sum() + (gR * G[1]).sum()).backward()
        assert dleaf.grad is None and frame.grad.shape == frame.shape and frame.grad.dtype == torch.float32
        for b in range(2):
            alpha = layers_from_rgbd(depth[b, 0], zs)
            den = lens.render_layers(frame0[b], alpha, zs, scales=scales, return_sums=True, **kw)[3]
            _, ht, _, bt = hand_grads(lens, frame0[b].contiguous(), alpha, zs, scales, x2, y2, G[:, b], den, DP, WVLN)
            assert_fp32_of(f"frame {b}", frame.grad[b], ht, bt)


# ------------------------------------------------------------------------------------ 7. the C entry
def _call_entry(lens, r, spp, trips, alpha, tex, depths, inv, gnum, galpha, gtex, stride=None):
    H, W = (int(v) for v in lens.sensor_res)
    K, L = len(lens.surfaces), len(depths)
    T, Ht, Wt = (int(v) for v in tex.shape[-3:])
    x1, y1 = sensor_axes(lens, True)
    x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
    assert x2.shape == (spp, H, W) and x2.dtype == torch.float32 and tex.is_contiguous() and L <= _lib.MAX_LAYERS
    assert gnum is None or (gnum.shape == (2, T, H, W) and gnum.dtype == torch.float64 and gnum.is_contiguous())
    pupilz, _ = lens.exit_pupil()
    dpp = C.byref(_lib.DpParams(*(float(v) for v in DP)))
    stride = (T * Ht * Wt if tex.dim() == 4 else 0) if stride is None else stride
    return _lib.lib().sdirt_render_layers_grad(
        lens.dev_lens(WVLN), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
        float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), spp, H, W, dpp, L, (C.c_double * L)(*depths),
        (C.c_double * L)(*inv), dptr(alpha), dptr(tex), T * Ht * Wt if tex.dim() == 4 else 0, T, Ht, Wt, dptr(gnum),
        dptr(galpha), dptr(gtex), stride, stream_ptr(lens.device))


def test_entry_accumulates_inside_its_slices_takes_nulls_and_refuses(lens, rays):
    """sdirt_render_layers_grad called directly with the forward's trip table, five planes (the second launch adds at
    an offset of four planes), both outputs slices between guard bands.  In-range arguments only.  Then what the host
    refuses: nothing is launched and the buffers keep what they held."""
    spp, n_tex, Ht, Wt, L = 8, 5, 2, 3, 3
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = (int(v) for v in lens.sensor_res)
        alpha = alpha_stack(L, Ht, Wt)
        tex = texture(L * n_tex, Ht, Wt, seed=82).view(L, n_tex, Ht, Wt)
        inv = layer_inv_texels(lens, depths, Wt)
        gnum = seeded_gnum(2, n_tex, H, W, seed=83)
        fwd = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN, landing=True)
        ref = reference(fwd["landing"], L, 2, alpha, tex, inv, gnum)
        ga, ga_ok = _guarded(L * Ht * Wt, torch.float64)
        gt, gt_ok = _guarded(L * n_tex * Ht * Wt, torch.float64)
        ga.zero_(), gt.zero_()
        for times in (1, 2):                                    # ADDED to: the second call doubles the buffers
            assert _call_entry(lens, r, spp, fwd["trips"], alpha, tex, depths, inv, gnum, ga, gt) == 0
            torch.cuda.synchronize()
            assert ga_ok() and gt_ok()
            assert_grads(f"call {times}", ga.view(L, Ht, Wt), gt.view(L, n_tex, Ht, Wt), ref, L, times=times)
        # either output null; the other is what it was with both
        only_a, only_t = torch.zeros(L, Ht, Wt, dtype=torch.float64, device=DEV), torch.zeros_like(tex, dtype=torch.float64)
        assert _call_entry(lens, r, spp, fwd["trips"], alpha, tex, depths, inv, gnum, only_a, None) == 0
        assert _call_entry(lens, r, spp, fwd["trips"], alpha, tex, depths, inv, gnum, None, only_t) == 0
        assert_grads("one output each", only_a, only_t, ref, L)
        # a shared gradient buffer under per-layer colours is not this entry's business; a shared texture is: stride 0
        shared_ref = reference(fwd["landing"], L, 2, alpha, tex[1], inv, gnum)
        shared_t = torch.zeros(n_tex, Ht, Wt, dtype=torch.float64, device=DEV)
        assert _call_entry(lens, r, spp, fwd["trips"], alpha, tex[1].contiguous(), depths, inv, gnum, None, shared_t) == 0
        assert_grads("stride 0", None, shared_t, shared_ref, L)
        # a null alpha: an opaque stack, only layer 0 is met
        opaque_ref = reference(fwd["landing"], L, 2, None, tex, inv, gnum)
        opaque_t = torch.zeros_like(tex, dtype=torch.float64)
        assert _call_entry(lens, r, spp, fwd["trips"], None, tex, depths, inv, gnum, None, opaque_t) == 0
        assert_grads("null alpha", None, opaque_t, opaque_ref, L)
        assert not opaque_t[1:].any()
        # refusals
        lib = _lib.lib()
        before_a, before_t = ga.clone(), gt.clone()

        def refused(msg, *a, **k):
            assert _call_entry(lens, r, spp, *a, **k) != 0
            assert msg in lib.sdirt_last_error(), lib.sdirt_last_error()

        ok = (fwd["trips"], alpha, tex, depths, inv, gnum, ga, gt)
        refused(b"null argument", *ok[:5], None, ga, gt)
        refused(b"both null", *ok[:6], None, None)
        refused(b"galpha without alpha", fwd["trips"], None, tex, depths, inv, gnum, ga, gt)
        refused(b"negative layer stride", *ok, stride=-1)
        for bad in ([-400.0, -400.0, -20000.0], [-400.0, -300.0, -20000.0], [400.0, -1000.0, -2000.0]):
            refused(b"strictly descending", fwd["trips"], alpha, tex, bad, inv, gnum, ga, gt)
        bad_trips = fwd["trips"].copy()
        bad_trips[0] = 99
        refused(b"trips[0]", bad_trips, alpha, tex, depths, inv, gnum, ga, gt)
        for n_layers in (0, 17):
            rc = lib.sdirt_render_layers_grad(lens.dev_lens(WVLN), None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum), dptr(gnum),
                                              0.0, 1, 1, 1, None, n_layers, (C.c_double * 17)(), (C.c_double * 17)(),
                                              dptr(alpha), dptr(tex), 0, 1, Ht, Wt, dptr(gnum), dptr(ga), dptr(gt), 0,
                                              stream_ptr(lens.device))
            assert rc != 0 and b"SDIRT_MAX_LAYERS" in lib.sdirt_last_error()
        rc = lib.sdirt_render_layers_grad(lens.dev_lens(WVLN), None, 0, dptr(gnum), dptr(gnum), 0.0, dptr(gnum), dptr(gnum), 0.0,
                                          0, 1, 1, None, 1, (C.c_double * 1)(-1.0), (C.c_double * 1)(1.0), dptr(alpha),
                                          dptr(tex), 0, 1, Ht, Wt, dptr(gnum), dptr(ga), dptr(gt), 0, stream_ptr(lens.device))
        assert rc != 0 and b"at least 1" in lib.sdirt_last_error()
        torch.cuda.synchronize()
        assert torch.equal(ga, before_a) and torch.equal(gt, before_t) and ga_ok() and gt_ok()


def test_a_side_stream_and_a_second_run_agree_within_the_bound(lens, rays):
    spp, L = 5, 3
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        alpha, tex = alpha_stack(L, 5, 141), texture(3, 5, 141, seed=83)
        inv = layer_inv_texels(lens, depths, 141)
        gnum = seeded_gnum(2, 3, H, W, seed=84)
        fwd, ga, gt = forward_and_grads(lens, alpha, tex, depths, inv, r, DP, gnum)
        ref = reference(fwd["landing"], L, 2, alpha, tex, inv, gnum)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(DEV) == side
            sa, st = layer_grad_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], fwd["trips"], gnum, DP, WVLN)
        side.synchronize()
        assert_grads("side stream", sa, st, ref, L)
        # two runs: the same terms in two arrival orders (not asserted bit-equal)
        for name, a, b in (("alpha", ga, sa), ("tex", gt, st)):
            bound = RG.bound(ref["n_" + name], L, ref["abs_" + name])
            assert (np.abs(a.cpu().numpy() - b.cpu().numpy()) <= bound).all()
            print(f"g{name}: the two runs are {'bit-equal' if torch.equal(a, b) else 'not bit-equal'}")
