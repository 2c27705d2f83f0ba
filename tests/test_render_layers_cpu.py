"""Ray-traced layered render, the parts that need no GPU: the C entry and its binding, the product's
float64 restatement (render_rt.layer_sums_float64, torch) against the independent one (tests/render_layers_f64.py,
numpy) on synthetic landings, its reduction to plane_sums_float64, layers_from_rgbd, and every argument error."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_lens
import render_layers_f64 as RL

ENTRY = "sdirt_render_layers"


def test_header_declares_the_entry_and_the_library_exports_it():
    import ctypes as C
    from sdirt_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, code)
    assert "#define SDIRT_ABI_VERSION 4" in txt and "#define SDIRT_MAX_LAYERS 16" in txt
    assert "DESIGN.md §7p" in txt
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    n_args = len(re.search(r"int\s+%s\s*\((.*?)\);" % ENTRY, code, re.S).group(1).split(","))
    assert restype is C.c_int and len(argtypes) == n_args == 28
    assert _lib.MAX_LAYERS == 16
    h = _lib.lib()
    assert hasattr(h, ENTRY)
    assert _lib.ABI_VERSION == 4 and h.sdirt_abi_version() == 4
    # a null lens is refused before anything touches a device
    assert h.sdirt_render_layers(None, None, 0, None, None, 0.0, None, None, 0.0, 1, 1, 1, None, 1, None, None, None,
                                 None, 0, 1, 1, 1, None, None, None, None, None, None) != 0
    assert b"null lens" in h.sdirt_last_error()


# ------------------------------------------------------------------------------------ restatement against restatement
H, W = 3, 37


def synthetic(L, Ht, Wt, S, seed, shared):
    """-> px, py [L, S, H, W], ra [S, H, W], w [2, S, H, W] fp32, alpha [L, Ht, Wt], tex ([L,] 3, Ht, Wt), inv [L].
    Landings reach 1.5 x the texture's half extent; a fifth of the rays are dead, every other of those on NaN, +-inf,
    +-3e38; alpha is 0 or 1 per texel, so a ray reads exactly 0, exactly 1 (four equal taps) or something between."""
    rng = np.random.default_rng(seed)
    inv = [0.37 * (1 + Wt) ** 0.5 * (1 + 0.21 * l) for l in range(L)]          # another texel size on every layer
    px = np.stack([rng.uniform(-1.5, 1.5, (S, H, W)) * (Wt / 2) / inv[l] for l in range(L)]).astype(np.float32)
    py = np.stack([rng.uniform(-1.5, 1.5, (S, H, W)) * (Ht / 2) / inv[l] for l in range(L)]).astype(np.float32)
    ra = (rng.uniform(size=(S, H, W)) >= 0.2).astype(np.float32)
    w = rng.uniform(0.0, 1.0, (2, S, H, W)).astype(np.float32)
    specials = [np.nan, np.inf, -np.inf, 3e38, -3e38]
    for n, idx in enumerate(np.flatnonzero(ra == 0)[::2]):
        for l in range(L):
            px[l].flat[idx] = specials[(n + l) % 5]
            py[l].flat[idx] = specials[(n // 5 + l) % 5]
    alpha = (rng.uniform(size=(L, Ht, Wt)) < 0.5).astype(np.float32)
    tex = rng.uniform(-0.25, 0.75, ((3, Ht, Wt) if shared else (L, 3, Ht, Wt))).astype(np.float32)
    return px, py, ra, w, alpha, tex, inv


def record(px, py, ra, w):
    """The landing record [3 + 2 L, S, H, W]: ra, w_L, w_R, px_0, py_0, ..."""
    rows = [ra, w[0], w[1]]
    for l in range(px.shape[0]):
        rows += [px[l], py[l]]
    return torch.from_numpy(np.stack(rows))


@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("shared", [False, True], ids=["per-layer", "shared"])
@pytest.mark.parametrize("L, Ht, Wt, S", [(1, 2, 3, 8), (2, 5, 141, 5), (3, 11, 280, 8), (5, 2, 3, 5), (16, 5, 9, 8)])
def test_the_product_s_restatement_equals_the_independent_one(L, Ht, Wt, S, shared, views):
    from sdirt_amd.render_rt import layer_sums_float64
    px, py, ra, w, alpha, tex, inv = synthetic(L, Ht, Wt, S, seed=100 * L + Wt + S, shared=shared)
    live = ra != 0
    assert 0.1 < 1 - live.mean() < 0.3
    for special in (np.isnan, np.isposinf, np.isneginf):
        assert special(px[:, ~live]).any() and not special(px[:, live]).any()
    _, _, a_all, T_before = RL.composite(px, py, ra, alpha, tex, inv)
    cls = RL.stack_classes(ra, a_all, T_before)
    print(f"L {L}, alpha {Ht} x {Wt}, S {S}: {cls}")
    assert cls["a0=0"] > 0.05 and cls["a0=1"] > 0.05 and cls["0<a0<1"] > 0.05, cls      # a_l of exactly 0 and 1
    if L > 1:
        assert cls["T=0 early"] > 0.05, cls
    if L < 16:
        assert cls["T never 0"] > 0.05, cls

    num, den, cov, ab, oab = RL.layer_sums_f64(px, py, ra, w[:views], alpha, tex, inv)
    assert num.shape == (views, 3, H, W) and den.shape == cov.shape == (views, H, W)
    got = layer_sums_float64(record(px, py, ra, w), torch.from_numpy(alpha), torch.from_numpy(tex), inv, views=views,
                             return_abs=True)
    pnum, pden, pcov, pab, poab = (t.numpy() for t in got)
    for arr in (num, den, cov, pnum, pden, pcov):
        assert np.isfinite(arr).all()
    eps = RL.sum_bound(S)
    worst = float((np.abs(num - pnum) / np.maximum(eps * ab, 1e-300)).max())
    print(f"worst |num - product's| / bound {worst:.3f}")
    assert (np.abs(num - pnum) <= eps * ab).all(), worst
    assert (np.abs(den - pden) <= eps * den).all()
    assert (np.abs(cov - pcov) <= eps * oab).all()
    assert (np.abs(ab - pab) <= eps * ab).all() and (np.abs(oab - poab) <= eps * oab).all()
    assert (den > 0).any() and (ab > 0).any() and (cov > 0).any() and (cov <= den).all()


def test_one_opaque_layer_is_the_plane_in_every_bit():
    """a_0 = w00 + w01 + w10 + w11 = 1 exactly (fu and fv are multiples of 2^-25 or so: every product and partial sum
    is exact in float64), so g = 1, c_k = t_k, T = 0, o = 1."""
    from sdirt_amd.render_rt import layer_sums_float64, plane_sums_float64
    for Ht, Wt, S in ((2, 3, 8), (5, 141, 5), (11, 280, 8)):
        px, py, ra, w, _, tex, inv = synthetic(1, Ht, Wt, S, seed=7 + Wt, shared=True)
        alpha = torch.ones(1, Ht, Wt)
        num, den, cov = layer_sums_float64(record(px, py, ra, w), alpha, torch.from_numpy(tex), inv)
        plane_record = torch.from_numpy(np.stack((px[0], py[0], ra, w[0], w[1])))
        pnum, pden = plane_sums_float64(plane_record, torch.from_numpy(tex), inv[0])
        assert torch.equal(num, pnum) and torch.equal(den, pden) and torch.equal(cov, den)
        # ... and so is a stack whose first layer is empty and whose second is opaque, with the second's texels
        px2, py2 = np.stack((px[0] * 0.5, px[0])), np.stack((py[0] * 0.5, py[0]))
        alpha2 = torch.stack((torch.zeros(Ht, Wt), torch.ones(Ht, Wt)))
        num2, den2, cov2 = layer_sums_float64(record(px2, py2, ra, w), alpha2, torch.from_numpy(tex), [3.0, inv[0]])
        assert torch.equal(num2, pnum) and torch.equal(den2, pden) and torch.equal(cov2, den2)


def test_compositing_worked_by_hand():
    """One pixel, 1 x 1 textures (every lookup is the texel), three layers with a = 0.5, 0.25, 1 and colours 1, 2, 4:
    c = 0.5 + 0.5 0.25 2 + 0.375 4 = 2.25, T = 0 -> o = 1.  Without the last layer T = 0.375, o = 0.625."""
    from sdirt_amd.render_rt import layer_sums_float64
    alpha = np.array([0.5, 0.25, 1.0], np.float32).reshape(3, 1, 1)
    tex = np.array([1.0, 2.0, 4.0], np.float32).reshape(3, 1, 1, 1)
    z = np.zeros((3, 1, 1, 1), np.float32)
    ra, w = np.ones((1, 1, 1), np.float32), np.array([0.5, 1.0], np.float32).reshape(2, 1, 1, 1)
    for fn in (lambda *a: RL.layer_sums_f64(*a)[:3],
               lambda px, py, ra, w, al, tx, inv: tuple(t.numpy() for t in layer_sums_float64(
                   record(px, py, ra, w), torch.from_numpy(al), torch.from_numpy(tx), inv))):
        num, den, cov = fn(z, z, ra, w, alpha, tex, [1.0, 1.0, 1.0])
        assert num[:, 0, 0, 0].tolist() == [0.5 * 2.25, 2.25] and den[:, 0, 0].tolist() == [0.5, 1.0]
        assert cov[:, 0, 0].tolist() == [0.5, 1.0]
        num, den, cov = fn(z[:2], z[:2], ra, w, alpha[:2], tex[:2], [1.0, 1.0])
        assert num[:, 0, 0, 0].tolist() == [0.5 * 0.75, 0.75] and cov[:, 0, 0].tolist() == [0.5 * 0.625, 0.625]


# ------------------------------------------------------------------------------------ layers_from_rgbd
def test_layers_from_rgbd_assigns_the_nearest_layer_in_inverse_depth():
    from sdirt_amd.render_rt import _check_layers, layers_from_rgbd, uniform_layer_depths
    zs = [-500.0, -1000.0, -4000.0]
    # 1/depth: -2e-3, -1e-3, -0.25e-3; midpoints at 1/depth = -1.5e-3 (-666.67) and -0.625e-3 (-1600)
    depth = torch.tensor([[-400.0, -600.0, -700.0], [-1500.0, -1700.0, -1e5]])
    own = torch.tensor([[0, 0, 1], [1, 2, 2]])
    hot = layers_from_rgbd(depth, zs, extend=False)
    assert hot.shape == (3, 2, 3) and hot.dtype == torch.float32
    assert torch.equal(hot.sum(0), torch.ones(2, 3)) and torch.equal(hot.argmax(0), own)       # one-hot
    ext = layers_from_rgbd(depth[None], zs)                                                     # [1, H, W] too
    assert torch.equal(ext, (torch.arange(3)[:, None, None] >= own[None]).float())
    assert bool((ext[1:] >= ext[:-1]).all()) and bool((ext[-1] == 1).all())                    # monotone, opaque at the back
    # a tie in 1/depth, exact in float64: 1/depth = -0.375 between layers at -0.5 and -0.25 -> the nearer layer
    d = -1.0 / 0.375
    assert 1.0 / d == -0.375 and abs(1.0 / d + 0.5) == abs(1.0 / d + 0.25)
    tie = layers_from_rgbd(torch.tensor([[d]], dtype=torch.float64), [-2.0, -4.0], extend=False)
    assert tie[:, 0, 0].tolist() == [1.0, 0.0]
    tie = layers_from_rgbd(torch.tensor([[d, d]], dtype=torch.float64), [-1.0, -2.0, -4.0, -8.0])
    assert tie[:, 0, 1].tolist() == [0.0, 1.0, 1.0, 1.0]
    assert uniform_layer_depths(torch.tensor([-700.0, -700.0]), 8) == [-700.0]
    u = uniform_layer_depths(torch.tensor([-500.0, -2000.0, -1000.0]), 4)
    assert u[0] == -500.0 and abs(u[-1] + 2000.0) < 1e-9 and np.allclose(np.diff(1 / np.asarray(u)), 0.5e-3)
    assert uniform_layer_depths(torch.tensor([-700.0, -2000.0]), 1) == [2.0 / (1.0 / -700.0 + 1.0 / -2000.0)]
    # a range below fp32's resolution at that depth (ulp(1000) = 6.1e-5): the layers that are equal once rounded are one
    tiny = torch.tensor([-1000.0, -1000.0001], dtype=torch.float64)
    for n in (1, 2, 8, 16):
        zs = uniform_layer_depths(tiny, n)
        z32 = np.asarray(zs, np.float32)
        assert 1 <= len(zs) <= n and bool((z32[1:] < z32[:-1]).all()) and (n == 1 or zs[0] == -1000.0), zs
        assert len(zs) <= 3                                     # two or three fp32 values lie in the range
        alpha = layers_from_rgbd(tiny[None], zs)
        assert alpha.shape == (len(zs), 1, 2) and bool((alpha[-1] == 1).all())
        _check_layers(alpha, torch.zeros(1, 1, 2), zs)          # what render_rgbd hands to render_layers is accepted
    for bad in ([-1000.0, -500.0], [-500.0, -500.0], [100.0], []):
        with pytest.raises(ValueError, match="strictly descending"):
            layers_from_rgbd(depth, bad)
    with pytest.raises(ValueError, match="must be negative"):
        layers_from_rgbd(-depth, zs)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        layers_from_rgbd(depth[None, None], zs)


# ------------------------------------------------------------------------------------ argument errors
def test_render_layers_and_render_rgbd_refuse_bad_arguments_before_anything_touches_the_gpu():
    from sdirt_amd import _lib
    from sdirt_amd.render_rt import layer_batch
    lens = make_lens("rf50mm", "cpu")
    lens.prepare_sensor(sensor_res=(4, 6), sensor_size=(1.0, 1.5))
    img, alpha, zs = torch.zeros(2, 3, 4, 6), torch.ones(2, 4, 6), [-500.0, -1000.0]
    kw = dict(scales=[5.0, 10.0])
    with pytest.raises(ValueError, match=r"\[L, C, Ht, Wt\]"):
        lens.render_layers(img[0, 0], alpha, zs, **kw)
    with pytest.raises(ValueError, match=r"alpha must be a \[L, Ht, Wt\]"):
        lens.render_layers(img, alpha[0], zs, **kw)
    with pytest.raises(ValueError, match="float32"):
        lens.render_layers(img.double(), alpha, zs, **kw)
    with pytest.raises(ValueError, match="float32"):
        lens.render_layers(img, alpha.double(), zs, **kw)
    with pytest.raises(ValueError, match="layers or extents differ"):
        lens.render_layers(img, torch.ones(2, 4, 5), zs, **kw)
    with pytest.raises(ValueError, match="layers or extents differ"):
        lens.render_layers(torch.zeros(3, 3, 4, 6), alpha, zs, **kw)
    for bad in (alpha * 1.5, alpha - 1.5, alpha * float("nan")):
        with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\]"):
            lens.render_layers(img, bad, zs, **kw)
    for bad in ([-1000.0, -500.0], [-500.0, -500.0], [500.0, -1000.0], [-500.0, -500.00001]):    # the last: equal in fp32
        with pytest.raises(ValueError, match="strictly descending"):
            lens.render_layers(img, alpha, bad, **kw)
    with pytest.raises(ValueError, match="2 layers need 2 depths"):
        lens.render_layers(img, alpha, [-500.0], scales=[5.0])
    with pytest.raises(ValueError, match="1 scales for 2 depths"):
        lens.render_layers(img, alpha, zs, scales=[5.0])
    with pytest.raises(ValueError, match="17 layers: between 1 and 16"):
        lens.render_layers(img[0], torch.ones(17, 4, 6), [-100.0 * (l + 1) for l in range(17)], scales=[1.0] * 17)
    with pytest.raises(ValueError, match="2 wavelengths for an image of 3 channels"):
        lens.render_layers(img, alpha, zs, wvln=[0.656, 0.486], **kw)
    with pytest.raises(ValueError, match="spp must be at least 1"):
        lens.render_layers(img, alpha, zs, spp=0, **kw)
    with pytest.raises(ValueError, match="pupil_points"):
        lens.render_layers(img, alpha, zs, spp=2, pupil_points=(torch.zeros(2, 4, 6), torch.zeros(3, 4, 6)), **kw)
    with pytest.raises(ValueError, match="alpha is on meta"):
        lens.render_layers(img, torch.ones(2, 4, 6, device="meta"), zs, **kw)
    pts = (torch.zeros(2, 4, 6), torch.zeros(2, 4, 6))
    # every argument in order, per-layer and shared image: the call gets as far as asking for the GPU
    for im in (img, img[0]):
        with pytest.raises(_lib.SdirtError, match="GPU only"):
            lens.render_layers(im, alpha, zs, spp=2, pupil_points=pts, **kw)
    with pytest.raises(ValueError, match="2 layers need 2 depths and 2 scales"):
        layer_batch(lens, alpha, img, zs, [1.0], *pts)
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        layer_batch(lens, alpha, img, zs, [1.0, 2.0], *pts)
    # render_rgbd
    frame, depth = torch.zeros(2, 3, 4, 6), torch.full((2, 1, 4, 6), -1000.0)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        lens.render_rgbd(frame[0], depth)
    for bad in (depth[:, 0], depth[:1], depth[..., :5], depth.expand(2, 2, 4, 6)):
        with pytest.raises(ValueError, match=r"depth must be \[B, 1, H, W\]"):
            lens.render_rgbd(frame, bad)
    for n in (0, 17):
        with pytest.raises(ValueError, match="n_layers must be between 1 and 16"):
            lens.render_rgbd(frame, depth, n_layers=n)
    with pytest.raises(ValueError, match="must be negative"):
        lens.render_rgbd(frame, -depth, scales=[10.0])
    with pytest.raises(ValueError, match="strictly descending"):
        lens.render_rgbd(frame, depth, layer_depths=[-1000.0, -500.0], scales=[10.0, 5.0])
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_rgbd(frame, depth, spp=2, scales=[10.0], pupil_points=pts)
    near_flat = depth.double().clone()
    near_flat[..., 3:] = -1000.0001                             # a valid frame whose range vanishes in fp32
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_rgbd(frame, near_flat, n_layers=8, spp=2, scales=[10.0] * 3, pupil_points=pts)      # three fp32 depths


def test_the_c_entry_validates_the_layers_on_the_host():
    """Null lens aside, the entry cannot be reached without a GPU lens handle; what it checks about the layers is
    restated by _check_layers, whose rounding to fp32 this pins: depths that differ in float64 only are refused."""
    from sdirt_amd.render_rt import _check_layers
    a, t = torch.ones(2, 1, 1), torch.zeros(1, 1, 1)
    assert _check_layers(a, t, [-500.0, -500.0001]) == (2, 1, 1, 1, True)
    with pytest.raises(ValueError, match="strictly descending"):
        _check_layers(a, t, [-500.0, -500.0000001])
