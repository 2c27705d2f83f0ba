"""k_render_layers (csrc/sdirt_render_rt.hip) on the GPU: a stack of fronto-parallel layers with
coverage, composited front to back along every ray.

  1. every layer's landing point, ray by ray, against the staged chain (trace, then propagate_to(z_l) on clones);
  2. its reduction to k_render_plane, bit for bit;
  3. its sums against tests/render_layers_f64.py (numpy, written from the text of §7p) within 2 S 2^-53 sum|term|;
  4. the sums of all 24 instantiations;
  5. occlusion at an opaque edge: exact colours on either side, a dual-pixel cue in between;
  6. render_layers / render_rgbd: chunks, wavelengths, the sums of one launch, a frame of one depth, a frame of two;
  7. a wrong bet on the trip table; the C entry with a null mask and a null landing record between guard bands; a stream.

Every class share below is evaluated on the STAGED chain's rays, never on the kernel's output.  rf50mm focused as in
test_gpu_render_raytraced.py; helpers and sensors come from there and from test_gpu_render_raytraced_edges.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_lens
import render_layers_f64 as RL
from render_rt_f64 import weights_f64
from test_gpu_render_raytraced import DP, DP_BIG, DEV, SMALL, WIDE, WVLN, pupil_points, same_bits, sensor
from test_gpu_render_raytraced_edges import (RAGGED, _guarded, assert_edges_live, half_cover_scale, inv_texel_of,
                                             magnification, texture)

from sdirt_amd import _lib
from sdirt_amd.basics import WAVE_RGB, Ray, dptr, stream_ptr
from sdirt_amd.render_rt import images_from_sums, layer_batch, layers_from_rgbd, plane_batch, sensor_axes

pytestmark = pytest.mark.gpu
FLOOR = 0.05
DEPTHS3 = (-400.0, -1000.0, -20000.0)


@pytest.fixture(scope="module")
def lens():
    m = make_lens("rf50mm", DEV)
    torch.manual_seed(0)
    m.focus_depth = -1000 + m.d_sensor
    m.refocus(m.focus_depth)
    return m


def stack_depths(L):
    """L depths uniform in 1 / depth from -400 to -20000 mm (one layer: -1000; three: about DEPTHS3's range)."""
    if L == 1:
        return [-1000.0]
    return [float(1.0 / v) for v in np.linspace(1.0 / -400.0, 1.0 / -20000.0, L)]


def staged_layers(lens, x2, y2, depths, pixel_center=True, wvln=WVLN):
    """The staged chain on the pupil points: Ray(o, o2 - o), trace (backward), then propagate_to(z_l) on a CLONE of the
    traced bundle for every layer -> px, py [L, S, H, W], ra [S, H, W], x_tan of the sampled direction, the trip table."""
    x1, y1 = sensor_axes(lens, pixel_center)
    gx, gy = torch.meshgrid(x1, y1, indexing="xy")
    o = torch.stack((gx, gy, torch.full_like(gx, lens.d_sensor)), 2)
    o2 = torch.stack((x2, y2, torch.full_like(x2, lens.exit_pupil()[0])), -1)
    ray = Ray(torch.broadcast_to(o, o2.shape), o2 - o, wvln=wvln, device=lens.device)
    shape, n = ray.shape, ray.numel
    d = ray.soa[3:6, :n].cpu().numpy()
    x_tan = (d[0] / -d[2]).reshape(shape)
    ray, _, _ = lens.trace(ray)
    K = len(lens.surfaces)
    trips = np.asarray(lens.trips.cache[("trace", round(wvln, 6), 0, K, False, lens.precision)])
    ra = ray.soa[6, :n].view(shape).clone()
    px, py = [], []
    for z in depths:
        at = ray.clone().propagate_to(z)
        px.append(at.soa[0, :n].view(shape).clone())
        py.append(at.soa[1, :n].view(shape).clone())
    return torch.stack(px), torch.stack(py), ra, x_tan, trips


def layer_inv_texels(lens, depths, Wt):
    """Every layer at the half-cover scale of the edges file: its texture spans the middle half of ITS landing range,
    so inv_texel differs from layer to layer."""
    return [inv_texel_of(lens, half_cover_scale(lens, z, lens.focus_depth), Wt) for z in depths]


def alpha_stack(L, Ht, Wt, seed=11, back=0.5):
    """Seeded random binary coverage per texel: a texel of layer 0 is covered with probability 1/2, one of the layers
    behind with probability `back`."""
    p = torch.full((L, 1, 1), back)
    p[0] = 0.5
    return (torch.rand(L, Ht, Wt, generator=torch.Generator().manual_seed(seed)) < p).float().to(DEV)


def land_points(land, L):
    return torch.stack([land[3 + 2 * l] for l in range(L)]), torch.stack([land[4 + 2 * l] for l in range(L)])


def restated(px, py, ra, w, alpha, tex, inv):
    out = RL.layer_sums_f64(*(a.cpu().numpy() for a in (px, py, ra, w, alpha, tex)), inv)
    return tuple(torch.from_numpy(a) for a in out)


def assert_sums(tag, out, ref, S):
    """num, den, cov of a launch against (num, den, cov, sum|wr c_k|, sum|wr o|) of the restatement."""
    rnum, rden, rcov, rabs, roabs = ref
    eps = RL.sum_bound(S)
    num, den, cov = (out[k].cpu() for k in ("num", "den", "cov"))
    assert num.shape == rnum.shape and den.shape == rden.shape and cov.shape == rcov.shape
    assert num.dtype == den.dtype == cov.dtype == torch.float64
    worst = [float(((a - b).abs() / (eps * c).clamp_min(1e-300)).max())
             for a, b, c in ((num, rnum, rabs), (den, rden, rden), (cov, rcov, roabs))]
    print(f"{tag}: worst |kernel - f64| / bound: num {worst[0]:.3f}, den {worst[1]:.3f}, cov {worst[2]:.3f}")
    assert bool(((num - rnum).abs() <= eps * rabs).all()), worst
    assert bool(((den - rden).abs() <= eps * rden).all()), worst
    assert bool(((cov - rcov).abs() <= eps * roabs).all()), worst
    assert bool((rden > 0).any()) and bool((rabs > 0).any()) and bool((rcov > 0).any())


@pytest.fixture(scope="module")
def rays(lens):
    """(spp, depths) -> the RAGGED bundle, pixel centres, lean: pupil points and the staged chain's landings on every
    layer.  Computed once per key, read only."""
    made = {}

    def get(spp, depths):
        key = (spp, tuple(depths))
        if key not in made:
            with sensor(lens, **RAGGED):
                x2, y2 = pupil_points(lens, spp, seed=200 + spp)
                px, py, ra, x_tan, trips = staged_layers(lens, x2, y2, depths)
            made[key] = dict(x2=x2, y2=y2, px=px, py=py, ra=ra, x_tan=x_tan, trips=trips)
        return made[key]
    return get


# ------------------------------------------------------------------------------------ 1. rays
@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("spp", [8, 5])                      # the stratified and the uniform branch of sample_pupil
def test_every_layer_s_landing_equals_the_staged_chain_bit_for_bit(lens, spp, precision):
    tol = 4 * DP[3] ** 2 * 3.1e-7                            # test 2 of test_gpu_render_raytraced.py: DESIGN.md §4
    L = len(DEPTHS3)
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        alpha, tex = alpha_stack(L, 2, 3), texture(3, 2, 3, seed=4)
        inv = layer_inv_texels(lens, DEPTHS3, 3)
        for centre, seed in ((False, 211), (True, 212)):
            x2, y2 = pupil_points(lens, spp, seed=seed)
            px, py, ra, x_tan, trips = staged_layers(lens, x2, y2, DEPTHS3, pixel_center=centre)
            dead = int((ra == 0).sum())
            print(f"{precision}, spp {spp}, {'centres' if centre else 'corners'}: {dead} of {ra.numel()} rays dead")
            assert 0 < dead < ra.numel() and bool(((ra == 0) | (ra == 1)).all())
            assert_edges_live(ra, H, W)
            out = layer_batch(lens, alpha, tex, DEPTHS3, inv, x2, y2, DP, WVLN, pixel_center=centre, landing=True)
            land = out["landing"]
            assert land.shape == (3 + 2 * L, spp, H, W) and land.dtype == torch.float32
            assert same_bits(land[0], ra)
            lx, ly = land_points(land, L)
            for l in range(L):
                assert same_bits(lx[l], px[l]) and same_bits(ly[l], py[l]), l
            assert not same_bits(lx[0], lx[1]) and not same_bits(lx[1], lx[2])
            assert np.array_equal(out["trips"], trips), (out["trips"], trips)
            # ... and each is k_render_plane's landing at that depth
            for l in (0, 2):
                pl = plane_batch(lens, tex, DEPTHS3[l], x2, y2, DP, WVLN, inv[l], pixel_center=centre, landing=True)
                assert same_bits(pl["landing"][0], lx[l]) and same_bits(pl["landing"][1], ly[l])
                assert same_bits(pl["landing"][2], land[0]) and same_bits(pl["landing"][3:5], land[1:3])
                assert np.array_equal(pl["trips"], out["trips"])
            # the weight rows: (w_L, w_R) = (sr, sl) of the float64 closed form
            sl, sr = weights_f64(x_tan, *DP)
            w = land[1:3].cpu().numpy()
            el, er = float(np.abs(w[0] - sr).max()), float(np.abs(w[1] - sl).max())
            print(f"  max |w_L - sr f64| {el:.3e}, max |w_R - sl f64| {er:.3e}, bound {tol:.3e}")
            assert np.abs(sr - sl).max() > 0.1 and el <= tol and er <= tol, (el, er, tol)
        # without dual-pixel parameters: one view, unit weight rows
        one = layer_batch(lens, alpha, tex, DEPTHS3, inv, x2, y2, None, WVLN, landing=True)
        assert one["num"].shape == (1, 3, H, W) and one["cov"].shape == (1, H, W)
        assert bool((one["landing"][1] == 1).all()) and bool((one["landing"][2] == 1).all())
        assert same_bits(one["landing"][3:], land[3:])


# ------------------------------------------------------------------------------------ 2. reduction to the plane kernel
@pytest.mark.parametrize("dp", [DP, None], ids=["dp", "none"])
@pytest.mark.parametrize("sens", [WIDE, RAGGED], ids=["wide", "ragged"])
@pytest.mark.parametrize("spp", [8, 5])
def test_an_opaque_layer_is_the_plane_kernel_s_plane_bit_for_bit(lens, spp, sens, dp):
    with sensor(lens, **sens):
        H, W = lens.sensor_res
        Ht, Wt = 7, 12
        depths = list(DEPTHS3)
        inv = layer_inv_texels(lens, depths, Wt)
        assert len(set(inv)) == 3
        x2, y2 = pupil_points(lens, spp, seed=220 + spp)
        tex = texture(3 * 5, Ht, Wt, seed=21).view(3, 5, Ht, Wt)          # five planes: a second launch
        behind = alpha_stack(3, Ht, Wt, seed=22)
        # (a) the first layer opaque, whatever lies behind
        alpha = behind.clone()
        alpha[0] = 1.0
        out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, dp, WVLN)
        pl = plane_batch(lens, tex[0], depths[0], x2, y2, dp, WVLN, inv[0])
        assert bool((pl["den"] > 0).any())
        assert torch.equal(out["num"], pl["num"]) and torch.equal(out["den"], pl["den"])
        assert torch.equal(out["cov"], out["den"]) and out["landing"] is None
        # (b) the first layer empty, the second opaque: the plane at z_1 with layer 1's texels and inv_texel
        alpha = behind.clone()
        alpha[0], alpha[1] = 0.0, 1.0
        out = layer_batch(lens, alpha, tex, depths, inv, x2, y2, dp, WVLN)
        pl = plane_batch(lens, tex[1], depths[1], x2, y2, dp, WVLN, inv[1])
        assert torch.equal(out["num"], pl["num"]) and torch.equal(out["den"], pl["den"])
        assert torch.equal(out["cov"], out["den"])
        assert not torch.equal(pl["num"], plane_batch(lens, tex[1], depths[1], x2, y2, dp, WVLN, inv[0])["num"])
        # a shared image (layer stride 0): the same plane behind every coverage
        out = layer_batch(lens, alpha, tex[1], depths, inv, x2, y2, dp, WVLN)
        assert torch.equal(out["num"], pl["num"]) and torch.equal(out["cov"], pl["den"])
        # nothing anywhere: black, den as before, no coverage
        out = layer_batch(lens, torch.zeros_like(alpha), tex, depths, inv, x2, y2, dp, WVLN)
        assert torch.equal(out["den"], pl["den"]) and not out["num"].any() and not out["cov"].any()


# ------------------------------------------------------------------------------------ 3. sums
# (layers, alpha texels, spp, colour per layer or shared, colour planes, share of covered texels behind layer 0).
# Sixteen layers of half-covered texels leave too few rays that never meet an opaque spot on the two large textures
# (3.5 % and 5.8 % of the live rays, measured on the staged chain): there the layers behind the first are covered to a
# fifth.  On 2 x 3 texels a quarter of the rays stays in one column pair, and the half-covered stack holds the floor.
CASES_3 = [(1, (2, 3), 8, False, 1, 0.5), (2, (5, 141), 5, False, 2, 0.5), (3, (11, 280), 8, True, 3, 0.5),
           (5, (2, 3), 5, False, 4, 0.5), (16, (5, 141), 8, False, 5, 0.2), (16, (11, 280), 5, True, 5, 0.2),
           (3, (2, 3), 8, True, 5, 0.5), (2, (11, 280), 8, False, 4, 0.5), (16, (2, 3), 8, True, 2, 0.5),
           (5, (5, 141), 5, True, 1, 0.5)]


@pytest.mark.parametrize("L, shape, spp, shared, planes, back", CASES_3)
def test_sums_equal_the_numpy_restatement(lens, rays, L, shape, spp, shared, planes, back):
    Ht, Wt = shape
    depths = stack_depths(L)
    r = rays(spp, depths)
    tag = f"L {L}, alpha {Ht} x {Wt}, spp {spp}, {'shared' if shared else 'per-layer'}, {planes} planes"
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        assert len(set(np.float32(inv).tolist())) == L           # another texel size on every layer
        alpha = alpha_stack(L, Ht, Wt, back=back)
        tex = texture(planes, Ht, Wt, seed=31) if shared else texture(L * planes, Ht, Wt, seed=32).view(L, planes, Ht, Wt)
        # the classes, on the staged chain's landings
        _, _, a_all, T_before = RL.composite(r["px"].cpu().numpy(), r["py"].cpu().numpy(), r["ra"].cpu().numpy(),
                                             alpha.cpu().numpy(), tex.cpu().numpy(), inv)
        cls = RL.stack_classes(r["ra"].cpu().numpy(), a_all, T_before)
        print(f"{tag}: shares of the live rays {cls}")
        assert cls["a0=0"] >= FLOOR and cls["0<a0<1"] >= FLOOR and cls["a0=1"] >= FLOOR, cls
        if L > 1:
            assert cls["T=0 early"] >= FLOOR, cls
            assert cls["T never 0"] >= FLOOR, cls
        else:                                                   # one layer: none before the last
            assert cls["T=0 early"] == 0 and cls["T never 0"] >= FLOOR, cls
        out = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN, landing=True)
        land = out["landing"]
        assert out["num"].shape == (2, planes, H, W) and out["den"].shape == out["cov"].shape == (2, H, W)
        lx, ly = land_points(land, L)
        assert same_bits(lx, r["px"]) and same_bits(ly, r["py"]) and same_bits(land[0], r["ra"])
        assert np.array_equal(out["trips"], r["trips"])
        ref = restated(r["px"], r["py"], r["ra"], land[1:3], alpha, tex, inv)
        assert_sums(tag, out, ref, spp)
        assert bool((out["cov"] <= out["den"]).all()) and not torch.equal(out["cov"], out["den"])
        # the same call without a landing record (lanes stop reading once T == 0): the same bits
        bare = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN)
        assert all(torch.equal(bare[k], out[k]) for k in ("num", "den", "cov"))


# ------------------------------------------------------------------------------------ 4. every instantiation
@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("dp", [None, DP, DP_BIG], ids=["none", "small", "big"])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_sums_of_every_instantiation(lens, rays, precision, dp, planes):
    """k_render_layers<M, DP, NT>: 2 x 3 x 4, at L = 2.  The restatement is fed with the launch's own landing record:
    what its rows hold is pinned by test 1 (and, for the big-radius weights, by test_gpu_render_raytraced.py through
    k_render_plane's record, which test 1 ties this one to)."""
    spp, Ht, Wt, L = 8, 7, 12, 2
    depths = stack_depths(L)
    r = rays(spp, depths)
    V = 1 if dp is None else 2
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        inv = layer_inv_texels(lens, depths, Wt)
        alpha = alpha_stack(L, Ht, Wt, seed=41)
        tex = texture(L * 4, Ht, Wt, seed=42).view(L, 4, Ht, Wt)[:, :planes].contiguous()
        out = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], dp, WVLN, landing=True)
        land = out["landing"]
        assert out["num"].shape == (V, planes, H, W) and out["den"].shape == out["cov"].shape == (V, H, W)
        lx, ly = land_points(land, L)
        if precision == "lean":
            assert same_bits(lx, r["px"]) and same_bits(ly, r["py"]) and same_bits(land[0], r["ra"])
        if dp is None:
            assert bool((land[1] == 1).all()) and bool((land[2] == 1).all())
        else:
            assert not torch.equal(land[1], land[2])
            assert 0 <= float(land[1:3].min()) and 0.1 < float(land[1:3].max()) <= 1
            pl = plane_batch(lens, tex[0], depths[0], r["x2"], r["y2"], dp, WVLN, inv[0], landing=True)["landing"]
            assert same_bits(pl[3:5], land[1:3])
        ref = restated(lx, ly, land[0], land[1:1 + V], alpha, tex, inv)
        assert_sums(f"{precision}, dp {dp}, {planes} planes", out, ref, spp)


# ------------------------------------------------------------------------------------ 5. occlusion
def test_an_opaque_edge_occludes_and_the_two_views_see_around_it_differently(lens):
    """An opaque half-plane (alpha_0 = 1 where px < 0: the right half of its texels) at -700 mm in front of an opaque
    background at -3000 mm, the lens focused at -1000 mm, on the 32 x 48 sensor of 1/32 mm pixels of
    test_gpu_render_raytraced.py (WIDE's and RAGGED's pixels are larger than the blur: no pixel would see both)."""
    z = [-700.0, -3000.0]
    spp = 8
    with sensor(lens, **SMALL):
        H, W = lens.sensor_res
        Ht, Wt = H, W
        scales = [magnification(lens, d, lens.focus_depth) for d in z]
        inv = [inv_texel_of(lens, s, Wt) for s in scales]
        alpha = torch.zeros(2, Ht, Wt, device=DEV)
        alpha[0, :, Wt // 2:] = 1.0                             # u = Wt/2 - px inv > Wt/2  <=>  px < 0
        alpha[1] = 1.0
        tex = torch.zeros(2, 2, Ht, Wt, device=DEV)             # one-hot colours: plane 0 foreground, plane 1 background
        tex[0, 0], tex[1, 1] = 1.0, 1.0
        x2, y2 = pupil_points(lens, spp, seed=51)
        px, _, ra, _, _ = staged_layers(lens, x2, y2, z)
        live = ra != 0
        assert bool(live.any(0).all())                          # every pixel has live rays
        texel = 1.0 / inv[0]
        big = torch.full_like(px[0], 1e30)
        fg = torch.where(live, px[0], -big).amax(0) < -texel    # all of the pixel's rays inside the half-plane
        bg = torch.where(live, px[0], big).amin(0) > texel      # all of them past its edge
        mid = ~(fg | bg)
        print(f"pixels: {int(fg.sum())} foreground, {int(bg.sum())} background, {int(mid.sum())} in between")
        assert int(fg.sum()) > 0.2 * H * W and int(bg.sum()) > 0.2 * H * W and int(mid.sum()) >= H
        img_L, img_R, num, den, cov = lens.render_layers(tex, alpha, z, spp=spp, dp=DP, wvln=WVLN, scales=scales,
                                                         pupil_points=(x2, y2), return_sums=True)
        assert torch.equal(cov, den)
        for v in (img_L, img_R):
            assert bool((v[0][fg] == 1).all()) and bool((v[1][fg] == 0).all())
            assert bool((v[0][bg] == 0).all()) and bool((v[1][bg] == 1).all())
            both = v.double().sum(0)
            assert float((both - 1).abs().max()) <= 2.0 ** -24 + 1e-12      # two fp32 roundings of values in [0, 1]
        # in between, the two views differ: the dual-pixel cue
        d =(img_R[0] - img_L[0])[mid]
        assert not torch.equal(img_L[0][mid], img_R[0][mid])
        print(f"foreground share, R - L over the {int(mid.sum())} pixels in between: mean {float(d.mean()):+.4f}, "
              f"largest |.| {float(d.abs().max()):.4f}, {int((d > 0).sum())} positive, {int((d < 0).sum())} negative")
        assert bool(((img_L[0] > 0) & (img_L[0] < 1))[mid].any())


# ------------------------------------------------------------------------------------ 6. render_layers, render_rgbd
def test_render_layers_chunks_wavelengths_and_sums(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        L, Ht, Wt = 3, 5, 9
        z = list(DEPTHS3)
        scales = [half_cover_scale(lens, d, lens.focus_depth) for d in z]
        inv = [inv_texel_of(lens, s, Wt) for s in scales]
        alpha = alpha_stack(L, Ht, Wt, seed=61)
        img = texture(L * 3, Ht, Wt, seed=62).view(L, 3, Ht, Wt)
        kw = dict(dp=DP, wvln=WVLN, scales=scales, return_sums=True)
        # 128 samples: the float64 sum of two 64-sample calls
        x2, y2 = pupil_points(lens, 128, seed=63)
        vL, vR, num, den, cov = lens.render_layers(img, alpha, z, spp=128, pupil_points=(x2, y2), **kw)
        a = lens.render_layers(img, alpha, z, spp=64, pupil_points=(x2[:64], y2[:64]), **kw)
        b = lens.render_layers(img, alpha, z, spp=64, pupil_points=(x2[64:], y2[64:]), **kw)
        assert num.shape == (2, 3, H, W) and den.shape == cov.shape == (2, H, W)
        assert torch.equal(num, a[2] + b[2]) and torch.equal(den, a[3] + b[3]) and torch.equal(cov, a[4] + b[4])
        want = images_from_sums(num, den.unsqueeze(1)).float()
        assert vL.shape == (3, H, W) and vL.dtype == torch.float32 and torch.equal(vL, want[0]) and torch.equal(vR, want[1])
        # the sums of one call of 8 samples are layer_batch's
        one = lens.render_layers(img, alpha, z, spp=8, pupil_points=(x2[:8], y2[:8]), **kw)
        part = layer_batch(lens, alpha, img, z, inv, x2[:8], y2[:8], DP, WVLN)
        assert all(torch.equal(one[2 + n], part[k]) for n, k in enumerate(("num", "den", "cov")))
        ph = lens.render_layers(img, alpha, z, spp=8, pupil_points=(x2[:8], y2[:8]), dp=DP, wvln=WVLN, scales=scales,
                                photometric=True)
        assert torch.equal(ph[0], (part["num"][0] / 8).float()) and torch.equal(ph[1], (part["num"][1] / 8).float())
        mono = lens.render_layers(img, alpha, z, spp=8, pupil_points=(x2[:8], y2[:8]), wvln=WVLN, scales=scales)
        assert torch.is_tensor(mono) and mono.shape == (3, H, W)
        # per-channel wavelengths, per-layer and shared image
        xs, ys = zip(*(pupil_points(lens, 8, seed=64 + c) for c in range(3)))
        x3, y3 = torch.stack(xs), torch.stack(ys)
        for im in (img, img[1]):
            cL, cR, cn, cd, cc = lens.render_layers(im, alpha, z, spp=8, dp=DP, wvln=WAVE_RGB, scales=scales,
                                                    pupil_points=(x3, y3), return_sums=True)
            assert cL.shape == (3, H, W) and cn.shape == cd.shape == cc.shape == (2, 3, H, W)
            for c in range(3):
                ch = im[:, c:c + 1] if im.dim() == 4 else im[c:c + 1]
                sL, sR, sn, sd, sc = lens.render_layers(ch.contiguous(), alpha, z, spp=8, dp=DP, wvln=WAVE_RGB[c],
                                                        scales=scales, pupil_points=(x3[c], y3[c]), return_sums=True)
                assert torch.equal(cL[c], sL[0]) and torch.equal(cR[c], sR[0])
                assert torch.equal(cn[:, c], sn[:, 0]) and torch.equal(cd[:, c], sd) and torch.equal(cc[:, c], sc)
            assert not torch.equal(cd[:, 0], cd[:, 2])


def test_render_rgbd_on_one_depth_is_render_plane_and_on_two_is_render_layers(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        frame = texture(2 * 3, H, W, seed=71).view(2, 3, H, W)
        x2, y2 = pupil_points(lens, 8, seed=72)
        kw = dict(spp=8, dp=DP, wvln=WVLN, pupil_points=(x2, y2))
        # one depth, one layer: the plane
        depth = torch.full((2, 1, H, W), -1500.0, device=DEV)
        scale = magnification(lens, -1500.0, lens.focus_depth)
        gL, gR = lens.render_rgbd(frame, depth, n_layers=1, scales=[scale], **kw)
        pL, pR = lens.render_plane(frame, -1500.0, scale=scale, **kw)
        assert gL.shape == (2, 3, H, W) and torch.equal(gL, pL) and torch.equal(gR, pR)
        assert float(gL.abs().max()) > 0
        # ... whatever n_layers asks for: a frame of one depth has one layer
        hL, hR = lens.render_rgbd(frame, depth, n_layers=8, scales=[scale], **kw)
        assert torch.equal(hL, pL) and torch.equal(hR, pR)
        # the default scale is calc_scale_ray's, which draws rays of its own: the same seed, the same image
        torch.manual_seed(5)
        dL, _ = lens.render_rgbd(frame[:1], depth[:1], n_layers=1, **kw)
        torch.manual_seed(5)
        qL, _ = lens.render_plane(frame[:1], -1500.0, **kw)
        assert torch.equal(dL, qL)
        one = lens.render_rgbd(frame, depth, n_layers=1, scales=[scale], spp=8, wvln=WVLN, pupil_points=(x2, y2))
        assert torch.is_tensor(one) and torch.equal(one, lens.render_plane(frame, -1500.0, scale=scale, spp=8, wvln=WVLN,
                                                                           pupil_points=(x2, y2)))
        # two depths: a near bar over a far background, another bar in the second frame
        depth = torch.full((2, 1, H, W), -3000.0, device=DEV)
        depth[0, 0, :, 20:40] = -700.0
        depth[1, 0, 1:, 5:30] = -700.0
        zs = [-700.0, -3000.0]
        scales = [magnification(lens, d, lens.focus_depth) for d in zs]
        gL, gR = lens.render_rgbd(frame, depth, n_layers=2, scales=scales, **kw)
        eL, eR = lens.render_rgbd(frame, depth, layer_depths=zs, scales=scales, **kw)
        assert torch.equal(gL, eL) and torch.equal(gR, eR)
        for b in range(2):
            alpha = layers_from_rgbd(depth[b, 0], zs)
            assert alpha.shape == (2, H, W) and bool((alpha[1] == 1).all()) and 0 < float(alpha[0].mean()) < 1
            wL, wR, _, den, cov = lens.render_layers(frame[b], alpha, zs, scales=scales, return_sums=True, **kw)
            assert torch.equal(gL[b], wL) and torch.equal(gR[b], wR) and torch.equal(cov, den)
        assert not torch.equal(gL[0], gL[1])
        # without `extend` rays fall through beside the bar: less coverage than light
        hot = lens.render_rgbd(frame, depth, layer_depths=zs, scales=scales, extend=False, **kw)
        assert not torch.equal(hot[0], gL)


# ------------------------------------------------------------------------------------ 7. trip table, entry, stream
def test_a_wrong_bet_on_the_trip_table_overwrites_the_outputs(lens, rays):
    spp, L, Ht, Wt = 8, 3, 2, 3
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        alpha, tex = alpha_stack(L, Ht, Wt), texture(5, Ht, Wt, seed=81)
        inv = layer_inv_texels(lens, depths, Wt)
        call = lambda: layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN, landing=True)
        warm = call()
        key = ("render_layers", round(WVLN, 6), lens.precision)
        good = lens.trips.cache[key].copy()
        assert np.array_equal(good, warm["trips"]) and np.array_equal(good, r["trips"])
        curved = lens._curved()
        k = max((i for i in range(len(good)) if curved[i]), key=lambda i: good[i])
        assert good[k] >= 2, good
        bad = good.copy()
        bad[k] -= 1
        lens.trips.cache[key] = bad
        lens.trips.votes[key] = {tuple(int(x) for x in bad): 99}
        before = lens.trips.relaunches
        try:
            again = call()
        finally:
            lens.trips.votes[key] = {tuple(int(x) for x in good): 1}
        assert lens.trips.relaunches > before
        assert np.array_equal(again["trips"], good) and np.array_equal(lens.trips.cache[key], good)
        assert all(torch.equal(again[k], warm[k]) for k in ("num", "den", "cov"))
        assert same_bits(again["landing"], warm["landing"])


def _call_entry(lens, r, spp, trips, alpha, tex, depths, inv, num, den, cov, land):
    H, W = (int(v) for v in lens.sensor_res)
    K, L = len(lens.surfaces), len(depths)
    T, Ht, Wt = (int(v) for v in tex.shape[-3:])
    x1, y1 = sensor_axes(lens, True)
    x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
    assert x2.shape == (spp, H, W) and x2.dtype == torch.float32 and tex.is_contiguous() and alpha.is_contiguous()
    assert alpha.shape == (L, Ht, Wt) and len(inv) == L and L <= _lib.MAX_LAYERS
    pupilz, _ = lens.exit_pupil()
    dpp = C.byref(_lib.DpParams(*(float(v) for v in DP)))
    _lib.check(_lib.lib().sdirt_render_layers(
        lens.dev_lens(WVLN), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
        float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), spp, H, W, dpp, L, (C.c_double * L)(*depths),
        (C.c_double * L)(*inv), dptr(alpha), dptr(tex), T * Ht * Wt if tex.dim() == 4 else 0, T, Ht, Wt, dptr(num),
        dptr(den), dptr(cov), dptr(land), None, stream_ptr(lens.device)))


def test_entry_writes_inside_its_slices_only_and_takes_null_mask_and_landing(lens, rays):
    """sdirt_render_layers called directly with the verified trip table, mask = NULL, five planes (the second launch
    writes num at an offset of four planes), every output a slice between guard bands; once with a landing record and
    once with landing = NULL.  In-range arguments only.  Then what the host refuses."""
    spp, n_tex, Ht, Wt, L = 8, 5, 2, 3, 3
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        H, W = (int(v) for v in lens.sensor_res)
        alpha = alpha_stack(L, Ht, Wt)
        tex = texture(L * n_tex, Ht, Wt, seed=82).view(L, n_tex, Ht, Wt)
        inv = layer_inv_texels(lens, depths, Wt)
        ref = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN, landing=True)
        for with_landing in (True, False):
            num, num_ok = _guarded(2 * n_tex * H * W, torch.float64)
            den, den_ok = _guarded(2 * H * W, torch.float64)
            cov, cov_ok = _guarded(2 * H * W, torch.float64)
            land, land_ok = _guarded((3 + 2 * L) * spp * H * W, torch.float32)
            _call_entry(lens, r, spp, ref["trips"], alpha, tex, depths, inv, num, den, cov, land if with_landing else None)
            torch.cuda.synchronize()
            assert num_ok() and den_ok() and cov_ok() and land_ok()
            assert torch.equal(num.view(2, n_tex, H, W), ref["num"]) and torch.equal(den.view(2, H, W), ref["den"])
            assert torch.equal(cov.view(2, H, W), ref["cov"])
            if with_landing:
                assert same_bits(land.view(3 + 2 * L, spp, H, W), ref["landing"])
            else:
                assert bool((land == -777.0).all())
        # the host's checks of the layers: nothing is launched, the outputs keep their sentinels
        for bad_depths in ([-400.0, -400.0, -20000.0], [-400.0, -300.0, -20000.0], [400.0, -1000.0, -2000.0]):
            with pytest.raises(_lib.SdirtError, match="strictly descending"):
                _call_entry(lens, r, spp, ref["trips"], alpha, tex, bad_depths, inv, num, den, cov, None)
        lib = _lib.lib()
        for n_layers in (0, 17):
            rc = lib.sdirt_render_layers(lens.dev_lens(WVLN), None, 0, dptr(num), dptr(num), 0.0, dptr(num), dptr(num), 0.0,
                                         1, 1, 1, None, n_layers, (C.c_double * 17)(), (C.c_double * 17)(), dptr(alpha),
                                         dptr(tex), 0, 1, Ht, Wt, dptr(num), dptr(den), dptr(cov), None, None,
                                         stream_ptr(lens.device))
            assert rc != 0 and b"SDIRT_MAX_LAYERS" in lib.sdirt_last_error()
        torch.cuda.synchronize()
        assert torch.equal(num.view(2, n_tex, H, W), ref["num"])


def test_a_side_stream_gives_the_same_bits(lens, rays):
    spp, L = 5, 3
    depths = list(DEPTHS3)
    r = rays(spp, depths)
    with sensor(lens, **RAGGED):
        alpha, tex = alpha_stack(L, 5, 141), texture(3, 5, 141, seed=83)
        inv = layer_inv_texels(lens, depths, 141)
        ref = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN, landing=True)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(DEV) == side
            out = layer_batch(lens, alpha, tex, depths, inv, r["x2"], r["y2"], DP, WVLN, landing=True)
        side.synchronize()
        assert all(torch.equal(out[k], ref[k]) for k in ("num", "den", "cov"))
        assert same_bits(out["landing"], ref["landing"]) and np.array_equal(out["trips"], ref["trips"])
