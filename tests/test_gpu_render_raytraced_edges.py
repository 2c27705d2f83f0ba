"""k_render_plane (csrc/sdirt_render_rt.hip) past what tests/test_gpu_render_raytraced.py reaches:
more than one workgroup and a ragged last one, textures of other extents than the sensor's with replicate addressing
on every side, the sums of all 24 instantiations, other lenses, planes and wavelengths, a wrong bet on the trip table,
output slices between guard bands with a null mask, a side stream.

The sums are checked against tests/render_rt_f64.py (numpy, written from the text of §7o, tied to the product's own
restatement by tests/test_render_rt_f64_cpu.py) within 2 S 2^-53 sum|term|; rays against the staged chain bit for
bit.  Every class share below is evaluated on the STAGED chain's rays, never on the kernel's output.

rf50mm focused as in test_gpu_render_raytraced.py, whose helpers this file imports."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_lens
import render_rt_f64 as R
from test_gpu_render_raytraced import DP, DP_BIG, DEPTH, DEV, WVLN, finish_staged, pupil_points, same_bits, sensor, staged

from sdirt_amd import _lib
from sdirt_amd.basics import dptr, stream_ptr
from sdirt_amd.render_rt import plane_batch, sensor_axes

pytestmark = pytest.mark.gpu
# 705 pixels of 0.25 mm: two full workgroups of 256 and 193 lanes (three waves and one lane); a row of 141 pixels
# straddles waves and workgroups; the field is as wide as WIDE's (+-17.6 mm), so some rays die in the lens
RAGGED = dict(res=(5, 141), size=(1.25, 35.25))
EDGE_PIXELS = (255, 256, 511, 512, 704)                      # last / first lanes of the workgroups, the last pixel
TEX_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 141), (11, 280)]
FLOOR = 0.05


@pytest.fixture(scope="module")
def lens():
    m = make_lens("rf50mm", DEV)
    torch.manual_seed(0)
    m.focus_depth = -1000 + m.d_sensor
    m.refocus(m.focus_depth)
    return m


def magnification(lens, depth, focus=None):
    """Object height per sensor height of a thin lens of lens.foclen focused at `focus` (default: at `depth` itself):
    -depth / v0 with v0 = f s0 / (s0 - f), as test 7 of test_gpu_render_raytraced.py computes it."""
    f = lens.foclen
    s0 = -(depth if focus is None else focus)
    return -depth / (f * s0 / (s0 - f))


def half_cover_scale(lens, depth, focus=None):
    """render_plane's `scale` for which the texture covers the middle half of the landing range along x: the sensor's
    width lands on magnification x width, the texture spans scale x width."""
    return 0.5 * magnification(lens, depth, focus)


def inv_texel_of(lens, scale, Wt):
    """render_plane's own expression: the same double, so plane_batch gets the same fp32 argument."""
    return 1.0 / (float(scale) * lens.pixel_size * int(lens.sensor_res[1]) / Wt)


def texture(T, Ht, Wt, seed):
    return (torch.rand(T, Ht, Wt, generator=torch.Generator().manual_seed(seed)) - 0.25).to(DEV)


def restated(px, py, ra, w, tex, inv):
    """tests/render_rt_f64.py on device tensors -> num, den, sum|term| as float64 tensors on the CPU."""
    out = R.plane_sums_f64(*(a.cpu().numpy() for a in (px, py, ra, w)), tex.cpu().numpy(), inv)
    return tuple(torch.from_numpy(a) for a in out)


def assert_sums(tag, num, den, rnum, rden, rabs, S):
    eps = R.sum_bound(S)
    num, den = num.cpu(), den.cpu()
    worst = float(((num - rnum).abs() / (eps * rabs).clamp_min(1e-300)).max())
    worst_den = float(((den - rden).abs() / (eps * rden).clamp_min(1e-300)).max())
    print(f"{tag}: worst |num - f64| / bound {worst:.3f}, |den - f64| / bound {worst_den:.3f}")
    assert num.shape == rnum.shape and den.shape == rden.shape
    assert bool(((num - rnum).abs() <= eps * rabs).all()), worst
    assert bool(((den - rden).abs() <= eps * rden).all()), worst_den
    assert bool((rden > 0).any()) and bool((rabs > 0).any())


def assert_edges_live(ra, H, W):
    """Rows 0 and H - 1 and the pixels at the workgroups' seams hold live rays (evaluated on the staged chain's ra)."""
    live = (ra != 0).any(0).reshape(-1).cpu()
    per_pixel = (ra != 0).sum(0).reshape(-1).cpu()
    print("live rays of pixels", EDGE_PIXELS, ":", [int(per_pixel[p]) for p in EDGE_PIXELS],
          f"; row 0: {int(per_pixel[:W].sum())}, row {H - 1}: {int(per_pixel[-W:].sum())}")
    assert H * W == 705 and all(bool(live[p]) for p in EDGE_PIXELS), per_pixel[list(EDGE_PIXELS)]
    assert bool(live[:W].any()) and bool(live[-W:].any())


@pytest.fixture(scope="module")
def rays(lens):
    """spp -> the RAGGED bundle of (a), pixel centres, lean: pupil points, the staged chain's px, py, ra and trips, and
    the fused launch's landing record under DP.  Computed once per spp, read only."""
    made = {}

    def get(spp):
        if spp not in made:
            with sensor(lens, **RAGGED):
                x2, y2 = pupil_points(lens, spp, seed=100 + spp)
                px, py, ra, x_tan, trips = staged(lens, x2, y2, DEPTH, pixel_center=True)
                tex = torch.zeros(1, 1, 1, device=DEV)
                land = plane_batch(lens, tex, DEPTH, x2, y2, DP, WVLN, 1.0, landing=True)["landing"]
            made[spp] = dict(x2=x2, y2=y2, px=px, py=py, ra=ra, x_tan=x_tan, trips=trips, land=land)
        return made[spp]
    return get


# ------------------------------------------------------------------------------------ a. rays past one workgroup
@pytest.mark.parametrize("precision", ["lean", "ieee"])
@pytest.mark.parametrize("spp", [8, 5])
def test_rays_of_three_workgroups_equal_the_staged_chain_bit_for_bit(lens, spp, precision):
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        tex = texture(3, 2, 3, seed=4)
        # pixel corners: sample_sensor() itself draws what pupil_points draws from the same seed
        x2, y2 = pupil_points(lens, spp, seed=111)
        torch.manual_seed(111)
        ray = lens.sample_sensor(spp=spp, wvln=WVLN)
        assert ray.shape == (spp, H, W)
        px, py, ra, _, trips = finish_staged(lens, ray, DEPTH)
        for centre, seed in ((False, 111), (True, 112)):
            if centre:
                x2, y2 = pupil_points(lens, spp, seed=seed)
                px, py, ra, _, trips = staged(lens, x2, y2, DEPTH, pixel_center=True)
            dead = int((ra == 0).sum())
            print(f"{precision}, spp {spp}, {'centres' if centre else 'corners'}: {dead} of {ra.numel()} rays dead")
            assert 0 < dead < ra.numel(), dead
            assert bool(((ra == 0) | (ra == 1)).all())
            assert_edges_live(ra, H, W)
            out = plane_batch(lens, tex, DEPTH, x2, y2, DP, WVLN, 0.5, pixel_center=centre, landing=True)
            land = out["landing"]
            assert land.shape == (5, spp, H, W)
            assert same_bits(land[2], ra)
            assert same_bits(land[0], px) and same_bits(land[1], py)
            assert np.array_equal(out["trips"], trips), (out["trips"], trips)


def test_the_shared_bundle_is_the_staged_chain_s(lens, rays):
    """The bundle tests b, c, d, f, g and h run on: pinned like any other, edge pixels live, and its weight rows are
    (w_L, w_R) = (sr, sl) of the float64 closed form within the 4 r^2 3.1e-7 of test_gpu_render_raytraced.py (DESIGN.md
    §4's bound on one segment area, four of them) -- the sums below are restated FROM these rows, so which row is
    which is settled here."""
    tol = 4 * DP[3] ** 2 * 3.1e-7
    for spp in (8, 5):
        r = rays(spp)
        sl, sr = R.weights_f64(r["x_tan"], *DP)
        w = r["land"][3:5].cpu().numpy()
        el, er = float(np.abs(w[0] - sr).max()), float(np.abs(w[1] - sl).max())
        print(f"spp {spp}: max |w_L - sr f64| {el:.3e}, max |w_R - sl f64| {er:.3e}, bound {tol:.3e}; "
              f"max |sr - sl| {np.abs(sr - sl).max():.3f}")
        assert np.abs(sr - sl).max() > 0.1                      # exchanged rows would miss the bound by far
        assert el <= tol and er <= tol, (el, er, tol)
        assert_edges_live(r["ra"], 5, 141)
        assert 0 < int((r["ra"] == 0).sum()) < r["ra"].numel()
        assert same_bits(r["land"][0], r["px"]) and same_bits(r["land"][1], r["py"]) and same_bits(r["land"][2], r["ra"])


# ------------------------------------------------------------------------------------ b. texture shapes, replicate
# Rows the geometry permits.  The sensor is 1.25 mm tall and the texel as large as it must be for Wt texels to span
# half of 35.25 mm: in texels the landings reach +-0.625 / (17.625 / Wt) = +-0.0355 Wt about the texture's middle row
# coordinate b = Ht/2 - 0.5 (thin lens; r0 = floor(b)).
#   (1, 1): b in +-0.04 -> r0 in {-1, 0}: below 0 and at the last row (n - 1 = 0), no pair inside
#   (1, 7): b in +-0.25 -> the same two
#   (7, 1): b in 3 +- 0.04 -> r0 in {2, 3}: inside only
#   (2, 3): b in 0.5 +- 0.11 -> r0 = 0: inside only
#   (5, 141): b in 2 +- 5 -> all three;  (11, 280): b in 5 +- 9.9 -> all three
LO, MID, HI = 0, 1, 2
Y_CLASSES = {(1, 1): (LO, HI), (1, 7): (LO, HI), (7, 1): (MID,), (2, 3): (MID,), (5, 141): (LO, MID, HI),
             (11, 280): (LO, MID, HI)}


def assert_classes(tag, r, inv, Ht, Wt):
    live = (r["ra"] != 0).cpu().numpy()
    px, py = (np.where(live, r[k].cpu().numpy(), 0) for k in ("px", "py"))
    c0, r0, _, _ = R.tap_origin(px, py, inv, Ht, Wt)
    xs, ys = R.tap_classes(c0, Wt, live), R.tap_classes(r0, Ht, live)
    print(f"{tag}: inv_texel {inv:.5f}; x classes < 0: {xs[0]:.3f}  0..n-2: {xs[1]:.3f}  >= n-1: {xs[2]:.3f};  "
          f"y classes {ys[0]:.3f} {ys[1]:.3f} {ys[2]:.3f}")
    # along x every class a texture of Wt texels has (one texel has no pair of distinct taps)
    assert xs[LO] >= FLOOR and xs[HI] >= FLOOR, xs
    assert xs[MID] >= FLOOR if Wt > 1 else xs[MID] == 0, xs
    for c in (LO, MID, HI):
        assert ys[c] >= FLOOR if c in Y_CLASSES[(Ht, Wt)] else ys[c] == 0, (c, ys)


@pytest.mark.parametrize("spp", [8, 5])
@pytest.mark.parametrize("Ht, Wt", TEX_SHAPES)
def test_texture_of_any_extent_with_replicate_addressing(lens, rays, Ht, Wt, spp):
    r = rays(spp)
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        scale = half_cover_scale(lens, DEPTH, lens.focus_depth)
        inv = inv_texel_of(lens, scale, Wt)
        tag = f"tex {Ht} x {Wt}, spp {spp}"
        assert_classes(tag, r, inv, Ht, Wt)
        img = texture(3, Ht, Wt, seed=10 * Ht + Wt).view(1, 3, Ht, Wt)
        tex = img[0]
        out = plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], DP, WVLN, inv, landing=True)
        num, den, land = out["num"], out["den"], out["landing"]
        assert num.shape == (2, 3, H, W) and den.shape == (2, H, W) and num.dtype == den.dtype == torch.float64
        assert same_bits(land, r["land"])                       # the rays do not depend on the texture
        rnum, rden, rabs = restated(r["px"], r["py"], r["ra"], land[3:5], tex, inv)
        assert_sums(tag, num, den, rnum, rden, rabs, spp)
        # the call: the same sums in every bit, the images their quotient rounded to fp32 once
        L, Rv, num2, den2 = lens.render_plane(img, DEPTH, spp=spp, dp=DP, wvln=WVLN, scale=scale,
                                              pupil_points=(r["x2"], r["y2"]), return_sums=True)
        assert num2.shape == (2, 1, 3, H, W) and torch.equal(num2.view(2, 3, H, W), num) and torch.equal(den2, den)
        d = den[:, None]
        want = torch.where(d > 0, num / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(num)).float()
        for got, v in ((L, 0), (Rv, 1)):
            assert got.shape == (1, 3, H, W) and got.dtype == torch.float32 and same_bits(got[0], want[v])


# ------------------------------------------------------------------------------------ c. one-hot textures
def test_one_hot_texels_light_their_own_corner_of_the_image(lens, rays):
    """The 2 x 3 texture as six one-hot planes (a four-plane launch and a two-plane launch over the same rays).  With
    the texture over the middle half of the landing range, texel (0, 0) -- top left -- is read by the pixels of the left
    half of the sensor (u = 1.5 - px inv <= 1.5, i.e. px >= 0, is where a tap can be on column 0) and weighs 1 - fv
    > 0.5 in the top rows (b = 0.5 - 0.11 there); (1, 2) mirrors it.  Rows and columns exchanged, or Ht taken for Wt,
    moves the light."""
    spp, Ht, Wt = 8, 2, 3
    r = rays(spp)
    with sensor(lens, **RAGGED):
        H, W = lens.sensor_res
        inv = inv_texel_of(lens, half_cover_scale(lens, DEPTH, lens.focus_depth), Wt)
        tex = torch.eye(6, device=DEV).view(6, Ht, Wt).contiguous()
        out = plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], DP, WVLN, inv, landing=True)
        num, den = out["num"], out["den"]
        rnum, rden, rabs = restated(r["px"], r["py"], r["ra"], out["landing"][3:5], tex, inv)
        assert_sums("one-hot 2 x 3", num, den, rnum, rden, rabs, spp)
        for k in range(6):
            assert bool(((num[:, k].cpu() - rnum[:, k]).abs() <= R.sum_bound(spp) * rabs[:, k]).all()), k
        live = r["ra"] != 0
        px = r["px"].double()
        margin = 1e-3                                           # mm on the plane, a texel is some 180 mm
        big = torch.full_like(px, 1e30)
        # a pixel none of whose live rays lands at px > -margin has no tap on column 0; at px < margin, none on column 2
        no_col0 = torch.where(live, px, -big).amax(0) < -margin
        no_col2 = torch.where(live, px, big).amin(0) > margin
        top, bottom, left, right = slice(0, H // 2), slice(H - H // 2, H), slice(0, W // 2), slice(W - W // 2, W)
        quadrants = {"tl": (top, left), "tr": (top, right), "bl": (bottom, left), "br": (bottom, right)}
        for k, own, dark in ((0, "tl", no_col0), (5, "br", no_col2)):
            assert 0.2 < float(dark.double().mean()) < 0.6, float(dark.double().mean())   # about half the sensor
            for v in range(2):
                img = torch.where(den[v] > 0, num[v, k] / den[v].clamp_min(1e-300), torch.zeros_like(den[v]))
                light = {q: float(img[rows, cols].sum()) for q, (rows, cols) in quadrants.items()}
                print(f"one-hot texel {divmod(k, Wt)}, view {v}: light per quadrant {light}, "
                      f"{int(dark.sum())} pixels without a tap on it")
                assert all(light[own] > light[q] for q in quadrants if q != own), light
                assert bool((num[v, k][dark] == 0).all()) and bool((num[v, k][~dark] != 0).any())


# ------------------------------------------------------------------------------------ d. every instantiation's sums
@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("dp", [None, DP, DP_BIG], ids=["none", "small", "big"])
@pytest.mark.parametrize("precision", ["lean", "ieee"])
def test_sums_of_every_instantiation(lens, rays, precision, dp, planes):
    """k_render_plane<M, DP, NT>: 2 x 3 x 4.  The restatement is fed with the launch's own landing record: what rows
    0..2 hold is pinned by (a), what rows 3 and 4 hold by the weight tests of test_gpu_render_raytraced.py."""
    spp, Ht, Wt = 8, 7, 12
    r = rays(spp)
    V = 1 if dp is None else 2
    with sensor(lens, precision=precision, **RAGGED):
        H, W = lens.sensor_res
        inv = inv_texel_of(lens, half_cover_scale(lens, DEPTH, lens.focus_depth), Wt)
        tex = texture(4, Ht, Wt, seed=77)[:planes].contiguous()
        out = plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], dp, WVLN, inv, landing=True)
        num, den, land = out["num"], out["den"], out["landing"]
        assert num.shape == (V, planes, H, W) and den.shape == (V, H, W)
        if precision == "lean":
            assert same_bits(land[:3], r["land"][:3])
        if dp is None:
            assert bool((land[3] == 1).all()) and bool((land[4] == 1).all())
        else:
            assert not torch.equal(land[3], land[4])
            assert 0 <= float(land[3:5].min()) and float(land[3:5].max()) <= 1 and float(land[3:5].max()) > 0.1
        rnum, rden, rabs = restated(land[0], land[1], land[2], land[3:3 + V], tex, inv)
        assert_sums(f"{precision}, dp {dp}, {planes} planes", num, den, rnum, rden, rabs, spp)


# ------------------------------------------------------------------------------------ e. other lenses, planes, colours
# Every case on RAGGED: the three prescriptions are full-frame lenses whose field ends near +-17.6 mm (0 < dead < all is
# asserted per case).
CASES_E = [("rf35mm", DEPTH, WVLN, True), ("rf50mm_variant", DEPTH, WVLN, True), ("rf50mm", -400.0, WVLN, False),
           ("rf50mm", -20000.0, WVLN, False), ("rf50mm", DEPTH, 0.486, False), ("rf50mm", DEPTH, 0.656, False)]


@pytest.mark.parametrize("name, depth, wvln, sums", CASES_E)
def test_other_lenses_planes_and_wavelengths(lens, name, depth, wvln, sums):
    m = lens if name == "rf50mm" else make_lens(name, DEV)
    spp, Ht, Wt = 8, 5, 9
    with sensor(m, **RAGGED):
        H, W = m.sensor_res
        inv = inv_texel_of(m, half_cover_scale(m, depth), Wt)
        tex = texture(3, Ht, Wt, seed=88)
        for precision in ("lean", "ieee"):
            m.precision = precision
            x2, y2 = pupil_points(m, spp, seed=120)
            px, py, ra, _, trips = staged(m, x2, y2, depth, pixel_center=True, wvln=wvln)
            dead = int((ra == 0).sum())
            print(f"{name} ({len(m.surfaces)} surfaces), depth {depth}, {wvln} um, {precision}: {dead} of {ra.numel()} "
                  f"rays dead, trips {trips.tolist()}")
            assert 0 < dead < ra.numel(), dead
            out = plane_batch(m, tex, depth, x2, y2, DP, wvln, inv, landing=True)
            land = out["landing"]
            assert same_bits(land[2], ra) and same_bits(land[0], px) and same_bits(land[1], py)
            assert np.array_equal(out["trips"], trips), (out["trips"], trips)
        if sums:
            live = (ra != 0).cpu().numpy()
            c0, r0, _, _ = R.tap_origin(*(np.where(live, a.cpu().numpy(), 0) for a in (px, py)), inv, Ht, Wt)
            print(f"{name}: x classes {R.tap_classes(c0, Wt, live)}, y classes {R.tap_classes(r0, Ht, live)}")
            rnum, rden, rabs = restated(px, py, ra, land[3:5], tex, inv)
            assert_sums(f"{name}, DP, 3 planes", out["num"], out["den"], rnum, rden, rabs, spp)


# ------------------------------------------------------------------------------------ f. a wrong bet on the trip table
def test_a_wrong_bet_on_the_trip_table_overwrites_the_outputs(lens, rays):
    spp = 8
    r = rays(spp)
    with sensor(lens, **RAGGED):
        tex = texture(5, 2, 3, seed=5)
        inv = inv_texel_of(lens, half_cover_scale(lens, DEPTH, lens.focus_depth), 3)
        call = lambda: plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], DP, WVLN, inv, landing=True)
        warm = call()
        key = ("render_plane", round(WVLN, 6), lens.precision)
        good = lens.trips.cache[key].copy()
        assert np.array_equal(good, warm["trips"]) and np.array_equal(good, r["trips"])
        curved = lens._curved()
        k = max((i for i in range(len(good)) if curved[i]), key=lambda i: good[i])
        assert good[k] >= 2, good                               # one trip short is still a table the kernel runs
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
        assert torch.equal(again["num"], warm["num"]) and torch.equal(again["den"], warm["den"])
        assert same_bits(again["landing"], warm["landing"])


# ------------------------------------------------------------------------------------ g. guard bands, null mask
def _guarded(n, dt, sentinel=-777.0, guard=4096):
    """A 16-byte-aligned slice of n elements in the middle of a sentinel-filled buffer -> (slice, check)."""
    whole = torch.full((guard + n + guard,), sentinel, dtype=dt, device=DEV)
    out = whole[guard:guard + n]
    assert out.data_ptr() % 16 == 0

    def untouched():
        return bool((whole[:guard] == sentinel).all()) and bool((whole[guard + n:] == sentinel).all())
    return out, untouched


def test_entry_writes_inside_its_slices_only_and_takes_a_null_mask(lens, rays):
    """sdirt_render_plane called directly with the verified trip table, mask = NULL, five planes (the second launch
    writes num at an offset of four planes), every output a slice between guard bands.  In-range arguments only."""
    spp, n_tex, Ht, Wt = 8, 5, 2, 3
    r = rays(spp)
    with sensor(lens, **RAGGED):
        H, W = (int(v) for v in lens.sensor_res)
        K = len(lens.surfaces)
        tex = texture(n_tex, Ht, Wt, seed=6)
        inv = inv_texel_of(lens, half_cover_scale(lens, DEPTH, lens.focus_depth), Wt)
        ref = plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], DP, WVLN, inv, landing=True)
        trips = ref["trips"]
        assert len(trips) == K
        num, num_ok = _guarded(2 * n_tex * H * W, torch.float64)
        den, den_ok = _guarded(2 * H * W, torch.float64)
        land, land_ok = _guarded(5 * spp * H * W, torch.float32)
        x1, y1 = sensor_axes(lens, True)
        x2, y2 = r["x2"].contiguous(), r["y2"].contiguous()
        assert x2.shape == (spp, H, W) and x2.dtype == torch.float32 and tex.is_contiguous()
        pupilz, _ = lens.exit_pupil()
        dpp = C.byref(_lib.DpParams(*(float(v) for v in DP)))
        _lib.check(_lib.lib().sdirt_render_plane(
            lens.dev_lens(WVLN), (C.c_int32 * K)(*[int(t) for t in trips]), lens._math_flags(), dptr(x1), dptr(y1),
            float(lens.d_sensor), dptr(x2), dptr(y2), float(pupilz), spp, H, W, dpp, float(DEPTH), float(inv), dptr(tex),
            n_tex, Ht, Wt, dptr(num), dptr(den), dptr(land), None, stream_ptr(lens.device)))
        torch.cuda.synchronize()
        assert num_ok() and den_ok() and land_ok()
        assert torch.equal(num.view(2, n_tex, H, W), ref["num"]) and torch.equal(den.view(2, H, W), ref["den"])
        assert same_bits(land.view(5, spp, H, W), ref["landing"])


# ------------------------------------------------------------------------------------ h. stream
def test_a_side_stream_gives_the_same_bits(lens, rays):
    spp = 5
    r = rays(spp)
    with sensor(lens, **RAGGED):
        tex = texture(3, 5, 141, seed=7)
        inv = inv_texel_of(lens, half_cover_scale(lens, DEPTH, lens.focus_depth), 141)
        ref = plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], DP, WVLN, inv, landing=True)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(DEV) == side
            out = plane_batch(lens, tex, DEPTH, r["x2"], r["y2"], DP, WVLN, inv, landing=True)
        side.synchronize()
        assert torch.equal(out["num"], ref["num"]) and torch.equal(out["den"], ref["den"])
        assert same_bits(out["landing"], ref["landing"]) and np.array_equal(out["trips"], ref["trips"])

