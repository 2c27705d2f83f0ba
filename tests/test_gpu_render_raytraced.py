"""Ray-traced rendering of a textured plane through the lens (csrc/sdirt_render_rt.hip) on the GPU:
the fused kernel ray by ray against the staged chain of the kernels it is made of (sample_sensor -> trace ->
propagate_to), its dual-pixel weights against the float64 closed form, its sums against the float64 restatement,
and the properties of the image: exact on a constant, additive over chunks of samples, per-channel wavelengths,
the dual-pixel disparity's sign on either side of focus, render_single_img.

rf50mm focused as the reference's fitting script focuses it (refocus(-1000 + d_sensor))."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import make_lens
from render_rt_f64 import weights_f64

from sdirt_amd.basics import WAVE_RGB, Ray
from sdirt_amd.render_rt import images_from_sums, plane_batch, plane_sums_float64, sensor_axes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DP = (0.78, 1.44, 0.3, 0.5)
DEPTH = -1000.0
WVLN = 0.589
# a row (70 pixels) crosses a wave's 64 pixels, and the field runs to +-17.5 mm, where rays miss the glass
WIDE = dict(res=(3, 70), size=(1.5, 35.0))
SMALL = dict(res=(32, 48), size=(1.0, 1.5))


@pytest.fixture(scope="module")
def lens():
    m = make_lens("rf50mm", DEV)
    torch.manual_seed(0)
    m.focus_depth = -1000 + m.d_sensor                       # the plane refocus() puts in focus
    m.refocus(m.focus_depth)
    return m


@contextlib.contextmanager
def sensor(lens, res, size, precision="lean"):
    keep = {k: getattr(lens, k) for k in ("sensor_res", "sensor_size", "pixel_size", "r_last", "precision")}
    lens.prepare_sensor(sensor_res=res, sensor_size=size)
    lens.precision = precision
    try:
        yield lens
    finally:
        for k, v in keep.items():
            setattr(lens, k, v)


def pupil_points(lens, spp, seed):
    torch.manual_seed(seed)
    pz, pr = lens.exit_pupil()
    o2 = lens.sample_pupil(lens.sensor_res, spp, pupilr=pr, pupilz=pz)
    return o2[..., 0].contiguous(), o2[..., 1].contiguous()


def staged(lens, x2, y2, depth, pixel_center, wvln=WVLN):
    """The parent's chain on the same pupil points: Ray(o, o2 - o), trace (backward), propagate_to(depth).
    -> (px, py, ra, x_tan of the sampled direction, the verified trip table), each ray array [S, H, W]."""
    x1, y1 = sensor_axes(lens, pixel_center)
    gx, gy = torch.meshgrid(x1, y1, indexing="xy")
    o = torch.stack((gx, gy, torch.full_like(gx, lens.d_sensor)), 2)
    o2 = torch.stack((x2, y2, torch.full_like(x2, lens.exit_pupil()[0])), -1)
    ray = Ray(torch.broadcast_to(o, o2.shape), o2 - o, wvln=wvln, device=lens.device)
    return finish_staged(lens, ray, depth, wvln)


def finish_staged(lens, ray, depth, wvln=WVLN):
    shape, n = ray.shape, ray.numel
    d = ray.soa[3:6, :n].cpu().numpy()
    x_tan = (d[0] / -d[2]).reshape(shape)                    # fp32, IEEE: monte_carlo.py:48 on the arriving direction -d
    lens.trace2obj(ray, depth)
    K = len(lens.surfaces)
    trips = lens.trips.cache[("trace", round(wvln, 6), 0, K, False, lens.precision)]
    px, py, ra = (ray.soa[r, :n].view(shape).clone() for r in (0, 1, 6))
    return px, py, ra, x_tan, np.asarray(trips)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. ray parity
@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("spp", [8, 5])                      # the stratified and the uniform branch of sample_pupil
def test_fused_rays_equal_the_staged_chain_bit_for_bit(lens, spp, precision):
    with sensor(lens, precision=precision, **WIDE):
        H, W = lens.sensor_res
        tex = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
        # pixel corners: against sample_sensor() itself, which draws what pupil_points drew from the same seed
        x2, y2 = pupil_points(lens, spp, seed=11)
        torch.manual_seed(11)
        ray = lens.sample_sensor(spp=spp, wvln=WVLN)
        assert ray.shape == (spp, H, W)
        px, py, ra, _, trips = finish_staged(lens, ray, DEPTH)
        dead = int((ra == 0).sum())
        assert 0 < dead < ra.numel(), dead                      # some rays die in the lens, not all
        assert bool(((ra == 0) | (ra == 1)).all())
        out = plane_batch(lens, tex, DEPTH, x2, y2, DP, WVLN, 0.5, pixel_center=False, landing=True)
        land = out["landing"]
        assert same_bits(land[2], ra)
        assert same_bits(land[0], px) and same_bits(land[1], py)
        assert np.array_equal(out["trips"], trips), (out["trips"], trips)
        # pixel centres (the renderer's default), other pupil points
        x2, y2 = pupil_points(lens, spp, seed=12)
        px, py, ra, _, trips = staged(lens, x2, y2, DEPTH, pixel_center=True)
        assert 0 < int((ra == 0).sum()) < ra.numel()
        out = plane_batch(lens, tex, DEPTH, x2, y2, DP, WVLN, 0.5, pixel_center=True, landing=True)
        land = out["landing"]
        assert same_bits(land[2], ra) and same_bits(land[0], px) and same_bits(land[1], py)
        assert np.array_equal(out["trips"], trips), (out["trips"], trips)


# ------------------------------------------------------------------------------------------------ 2. weights
def test_weights_are_the_closed_form_of_the_arriving_direction(lens):
    """A weight is r^2 times four segment areas plus a strip width, and DESIGN.md §4 bounds one area of the polynomial
    (seg_acos) by 3.1e-7 absolute against float64: 4 r^2 3.1e-7 for the weight, the bound taken from there."""
    h, f, w, r = DP
    tol = 4 * r * r * 3.1e-7
    with sensor(lens, **WIDE):
        tex = torch.zeros(1, *lens.sensor_res, device=DEV)
        for spp, seed in ((8, 21), (5, 22)):
            x2, y2 = pupil_points(lens, spp, seed)
            _, _, _, x_tan, _ = staged(lens, x2, y2, DEPTH, pixel_center=True)
            land = plane_batch(lens, tex, DEPTH, x2, y2, DP, WVLN, 0.5, landing=True)["landing"].cpu().numpy()
            sl, sr = weights_f64(x_tan, *DP)
            el, er = np.abs(land[3] - sr).max(), np.abs(land[4] - sl).max()      # (w_L, w_R) = (sr, sl): DESIGN.md §7o
            print(f"spp {spp}: |x_tan| <= {np.abs(x_tan).max():.3f}, max |w_L - f64| {el:.3e}, max |w_R - f64| {er:.3e}, "
                  f"bound {tol:.3e}")
            assert np.abs(x_tan).max() > 0.2                    # the field is wide: the weights are far from on-axis
            assert el <= tol and er <= tol, (el, er, tol)
        # without dual-pixel parameters: one view, unit weights
        land = plane_batch(lens, tex, DEPTH, x2, y2, None, WVLN, 0.5, landing=True)["landing"]
        assert bool((land[3] == 1).all()) and bool((land[4] == 1).all())


DP_BIG = (0.78, 1.44, 0.3, 0.6)                              # r > 0.5: dp_weights_big


def splat_weights(x_tan, dp, precision):
    """(sl, sr) of every x_tan as the STAGED SPLAT computes them (sdirt_forward_integral behind
    assign_points_to_pixels_small_r / _big_r): one ray of weight 1 on the centre of a pixel of its own in a 33 x 33
    grid of unit pixels (a power of two across: the tap position is an exact integer, the tap's weight exactly 1, the
    three other taps get 0 x sl), so the pixel holds the ray's sl (sr in the right grid) in every bit.  The outermost
    ring is outside the splat's window: 31 x 31 rays per call."""
    from sdirt_amd import assign_points_to_pixels_big_r, assign_points_to_pixels_small_r
    ks, side = 33, 31
    xt = torch.as_tensor(x_tan, dtype=torch.float32).reshape(-1).to(DEV)
    idx = torch.arange(side * side, device=DEV)
    cx, cy = (idx % side - 15).float(), (15 - idx // side).float()
    sl, sr = torch.empty_like(xt), torch.empty_like(xt)
    for n0 in range(0, xt.numel(), side * side):
        x = xt[n0:n0 + side * side]
        n = x.numel()
        kw = dict(points=torch.stack((cx[:n], cy[:n]), 1), ks=ks, x_range=[-16.0, 16.0], y_range=[-16.0, 16.0],
                  ra=torch.ones(n, device=DEV), x_tan=x, param_list=list(dp) + ["l"])
        l, r = assign_points_to_pixels_big_r(**kw) if dp[3] > 0.5 else assign_points_to_pixels_small_r(precision=precision, **kw)
        row, col = (16 - cy[:n]).long(), (cx[:n] + 16).long()
        sl[n0:n0 + n], sr[n0:n0 + n] = l[row, col], r[row, col]
        assert float(l.double().sum()) == float(l[row, col].double().sum())         # nothing landed anywhere else
        assert float(r.double().sum()) == float(r[row, col].double().sum())
    return sl, sr


@pytest.mark.parametrize("dp", [DP, DP_BIG])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_weights_are_the_staged_splat_s_in_every_bit(lens, dp, precision):
    """Small and big microlens radius, both math policies: the kernel calls the splat's own weight functions on the same
    fp32 x_tan, so its weights are the splat's bits (exchanged: (w_L, w_R) = (sr, sl)).  No tolerance."""
    with sensor(lens, precision=precision, **WIDE):
        tex = torch.zeros(4, *lens.sensor_res, device=DEV)      # four planes: the largest instantiation of each form
        x2, y2 = pupil_points(lens, 8, seed=23)
        _, _, _, x_tan, _ = staged(lens, x2, y2, DEPTH, pixel_center=True)
        land = plane_batch(lens, tex, DEPTH, x2, y2, dp, WVLN, 0.5, landing=True)["landing"]
        sl, sr = splat_weights(x_tan, dp, precision)
        assert float(sl.max()) > 0.1 and float(sr.max()) > 0.1 and not torch.equal(sl, sr)
        assert same_bits(land[3].reshape(-1), sr) and same_bits(land[4].reshape(-1), sl)


# ------------------------------------------------------------------------------------------------ 3. sums
@pytest.mark.parametrize("dp", [DP, None])
@pytest.mark.parametrize("spp", [8, 5])
def test_sums_equal_the_float64_restatement_and_the_images_are_their_quotient(lens, spp, dp):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        V = 2 if dp else 1
        # two RGB images = six planes sharing one trace: a launch of four planes and a second one of two over the same rays
        img = (torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(6)) - 0.25).to(DEV)
        tex = img.reshape(6, H, W)
        x2, y2 = pupil_points(lens, spp, seed=31)
        scale = 12.5
        inv = 1.0 / (scale * lens.pixel_size * W / W)
        out = plane_batch(lens, tex, DEPTH, x2, y2, dp, WVLN, inv, landing=True)
        num, den, land = out["num"], out["den"], out["landing"]
        assert num.shape == (V, 6, H, W) and den.shape == (V, H, W) and num.dtype == den.dtype == torch.float64
        rnum, rden, rabs = plane_sums_float64(land, tex, inv, views=V, return_abs=True)
        # every plane count a launch is compiled for, alone: the same sums of its planes, in every bit
        for t in (1, 2, 3, 4, 5):
            part = plane_batch(lens, tex[:t], DEPTH, x2, y2, dp, WVLN, inv)
            assert torch.equal(part["num"], num[:, :t]) and torch.equal(part["den"], den), t
        eps = 2 * spp * 2.0 ** -53                             # any summation order of S float64 terms
        assert bool(((num - rnum).abs() <= eps * rabs).all()), ((num - rnum).abs() / rabs.clamp_min(1e-300)).max()
        assert bool(((den - rden).abs() <= eps * rden).all())
        assert bool((den > 0).any())
        # the call itself: the same sums, and the images are their quotient rounded to fp32 once
        res = lens.render_plane(img, DEPTH, spp=spp, dp=dp, wvln=WVLN, scale=scale, pupil_points=(x2, y2), return_sums=True)
        views, (num2, den2) = res[:V], res[V:]
        assert num2.shape == (V, 2, 3, H, W) and torch.equal(num2.view(V, 6, H, W), num) and torch.equal(den2, den)
        want = images_from_sums(num, den).float()
        for v in range(V):
            assert views[v].shape == (2, 3, H, W) and views[v].dtype == torch.float32
            assert torch.equal(views[v].reshape(6, H, W), want[v])
        # photometric: num / spp
        ph = lens.render_plane(img, DEPTH, spp=spp, dp=dp, wvln=WVLN, scale=scale, pupil_points=(x2, y2), photometric=True)
        ph = ph if dp else (ph,)
        for v in range(V):
            assert torch.equal(ph[v].reshape(6, H, W), (num[v] / spp).float())


# ------------------------------------------------------------------------------------------------ 4. exactness
def test_a_constant_texture_renders_to_the_constant_exactly(lens):
    """Products with a power of two are exact: num = den / 2 in every bit."""
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        img = torch.full((1, 2, H, W), 0.5, device=DEV)
        x2, y2 = pupil_points(lens, 8, seed=41)
        L, R, num, den = lens.render_plane(img, DEPTH, spp=8, dp=DP, scale=12.5, pupil_points=(x2, y2), return_sums=True)
        lit = (den > 0)[:, None, None].expand(2, 1, 2, H, W)
        assert bool(lit.any())
        both = torch.stack((L, R))
        assert bool((both[lit] == 0.5).all()) and bool((both[~lit] == 0).all())
        assert torch.equal(num, (den * 0.5)[:, None, None].expand_as(num))


# ------------------------------------------------------------------------------------------------ 5. chunks
def test_a_call_above_64_samples_is_the_sum_of_its_chunks(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        img = torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(7)).to(DEV)
        x2, y2 = pupil_points(lens, 128, seed=51)
        kw = dict(dp=DP, wvln=WVLN, scale=12.5, return_sums=True)
        L, R, num, den = lens.render_plane(img, DEPTH, spp=128, pupil_points=(x2, y2), **kw)
        a = lens.render_plane(img, DEPTH, spp=64, pupil_points=(x2[:64], y2[:64]), **kw)
        b = lens.render_plane(img, DEPTH, spp=64, pupil_points=(x2[64:], y2[64:]), **kw)
        assert torch.equal(num, a[2] + b[2]) and torch.equal(den, a[3] + b[3])
        want = images_from_sums(num, den.view(2, 1, 1, H, W)).float()
        assert torch.equal(L, want[0]) and torch.equal(R, want[1])
        # ... and the same call gives the same bits
        again = lens.render_plane(img, DEPTH, spp=128, pupil_points=(x2, y2), **kw)
        assert torch.equal(again[2], num) and torch.equal(again[3], den)


# ------------------------------------------------------------------------------------------------ 6. chromatic
def test_channels_are_traced_at_their_own_wavelengths(lens):
    with sensor(lens, **WIDE):
        H, W = lens.sensor_res
        img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(8)).to(DEV)
        xs, ys = zip(*(pupil_points(lens, 8, seed=60 + c) for c in range(3)))
        x2, y2 = torch.stack(xs), torch.stack(ys)
        L, R, num, den = lens.render_plane(img, DEPTH, spp=8, dp=DP, wvln=WAVE_RGB, scale=12.5, pupil_points=(x2, y2),
                                           return_sums=True)
        assert L.shape == R.shape == (2, 3, H, W) and num.shape == (2, 2, 3, H, W) and den.shape == (2, 3, H, W)
        for c in range(3):
            Lc, Rc, nc, dc = lens.render_plane(img[:, c:c + 1], DEPTH, spp=8, dp=DP, wvln=WAVE_RGB[c], scale=12.5,
                                               pupil_points=(x2[c], y2[c]), return_sums=True)
            assert torch.equal(L[:, c], Lc[:, 0]) and torch.equal(R[:, c], Rc[:, 0])
            assert torch.equal(num[:, :, c], nc[:, :, 0]) and torch.equal(den[:, c], dc)
        assert not torch.equal(den[:, 0], den[:, 2])             # dispersion: the channels are not one trace


# ------------------------------------------------------------------------------------------------ 7. dual-pixel sign
def x_centroid(img):
    col = img.double().sum(dim=tuple(range(img.dim() - 1)))
    return float((col * torch.arange(col.numel(), device=col.device)).sum() / col.sum())


def test_dual_pixel_disparity_changes_sign_across_focus(lens):
    """A bright bar, two texels wide, on black, nearer than, at and farther than the focused plane.  Thin-lens estimate of
    the blur: with f = lens.foclen, the aperture D = f / lens.fnum, the focused object distance s0 and image distance
    v0 = f s0 / (s0 - f), an object at s images at v = f s / (s - f) and blurs to D |v - v0| / v on the sensor; the two
    planes are chosen for 4 to 8 pixels of 1 / 32 mm (asserted below)."""
    focus = lens.focus_depth
    near, far = -740.0, -1280.0
    with sensor(lens, **SMALL):
        H, W = lens.sensor_res
        f, D = lens.foclen, lens.foclen / lens.fnum
        v0 = f * -focus / (-focus - f)
        for depth in (near, far):
            v = f * -depth / (-depth - f)
            blur_px = D * abs(v - v0) / v / lens.pixel_size
            print(f"depth {depth}: thin-lens blur {blur_px:.2f} pixels")
            assert 4 <= blur_px <= 8, blur_px
        img = torch.zeros(1, 1, H, W, device=DEV)
        img[..., W // 2 - 1:W // 2 + 1] = 1.0
        got, want = {}, {}
        for depth in (near, focus, far):
            torch.manual_seed(70)
            L, R = lens.render_plane(img, depth, spp=64, dp=DP, wvln=WVLN, scale=-depth / v0)
            got[depth] = x_centroid(R) - x_centroid(L)
            pl, pr = lens.psf_lr(torch.tensor([[0.0, 0.0, depth]]), ks=31, wvln=WVLN, dp=DP)
            want[depth] = x_centroid(pr) - x_centroid(pl)
            print(f"depth {depth:9.2f}: centroid R - L = {got[depth]:+.4f} pixels rendered, {want[depth]:+.4f} of psf_lr")
        assert got[near] * got[far] < 0, got
        assert got[near] * want[near] > 0 and got[far] * want[far] > 0, (got, want)
        assert abs(got[focus]) < abs(got[near]) and abs(got[focus]) < abs(got[far]), got


# ------------------------------------------------------------------------------------------------ 8. render_single_img
def test_render_single_img_raytracing_is_render_plane_at_the_image_s_resolution(lens):
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    before = (lens.sensor_res, lens.sensor_size, lens.pixel_size, lens.r_last)
    torch.manual_seed(80)
    out = lens.render_single_img(img, depth=DEPTH, spp=8, method="raytracing")
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (16, 24, 3)
    assert (lens.sensor_res, lens.sensor_size, lens.pixel_size, lens.r_last) == before
    torch.manual_seed(80)
    t = lens.render_single_img(img, depth=DEPTH, spp=8, method="raytracing", return_tensor=True, noise=0)
    assert t.shape == (1, 3, 16, 24) and t.dtype == torch.float32
    assert np.array_equal(t[0].mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy(), out)
    with sensor(lens, res=[16, 24], size=(24.0, 36.0)):
        torch.manual_seed(80)
        tex = torch.tensor((img / 255.).astype(np.float32)).permute(2, 0, 1).unsqueeze(0).to(DEV)
        want = lens.render_plane(tex, DEPTH, spp=8, dp=None, wvln=WAVE_RGB, pixel_center=False)
    assert torch.equal(t, want)
    # the image is upright and no mirror image: it correlates with the texture, not with its flips
    err = lambda a: float((t - a).abs().mean())
    assert err(tex) < err(tex.flip(-1)) and err(tex) < err(tex.flip(-2)) and err(tex) < err(tex.flip(-1, -2))
