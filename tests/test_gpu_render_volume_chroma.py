"""local_dp_psf_render_volume with a CHROMATIC volume [C,Dz,Gy,Gx,2,ks,ks] on the GPU: the four k_*_chroma kernels of
sdirt_render_volume.hip against the float64 restatement (tests/render_volume_chroma_f64.py, which
tests/test_render_volume_chroma_cpu.py holds against the reference's local_dp_psf_render channel by channel) and, bit
for bit, against the achromatic kernels called at C = 1 on every channel's slices.  The operands are independent randn
per channel of the volume; the segment tables are computed once in fp32 and handed to both sides.

The bars are those derived in tests/test_gpu_render_volume.py and tests/test_gpu_render_volume_scene.py: they count
terms and roundings per term, and a volume per channel changes neither.  Unit 2^-23; sum|terms| is the same sum on the
operands' magnitudes:
  forward, per output element:  (8 ks^2 + 8) 2^-23 sum|terms|
  d volume, per element:        (n + 8) 2^-23 sum|terms|, n = the (b, pixel) with a non-zero weight at the node: an
      element of dV[c] sums one product G[c] P[c] per pixel, so C no longer multiplies n
  d image, per element:         (16 ks^2 m + 8) 2^-23 sum|terms|, m = the padded positions that clamp onto the element
  d fz, per pixel:              (16 C ks^2 + 8) 2^-23 sum|terms|: 2 * C * 8 * ks^2 terms, each with 1 rounding in the
      weight's derivative wy wx and 3 in the products (with V, with P, with G); the kernel folds nothing before the tap
      sum, which leaves the count of the achromatic bar (3 + 3 per term) untouched.
The collapse test compares the fp32 sum over the channels of dV with the float64 ACHROMATIC dV under the achromatic bar
(C n + 8): channel c errs by at most (n + 8) 2^-23 S_c, the C - 1 additions by 2^-23 S each, S = sum_c S_c the
achromatic sum|terms|, together at most (n + 8 + C - 1) 2^-23 S <= (C n + 8) 2^-23 S for n >= 1 (n = 0: both are 0)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from conftest import DATA, load_state, make_lens
from render_volume_chroma_f64 import (dfz_chroma_abs, dimg_chroma_abs, render_volume_chroma_abs,
                                      render_volume_chroma_f64, scene_grads_chroma_f64, volume_grad_chroma_abs,
                                      volume_grad_chroma_f64)
from render_volume_f64 import interpolate_kernels, node_pixel_counts, volume_grad_abs, volume_grad_f64
from render_volume_scene_f64 import fold_counts
from test_gpu_render_volume import depth_map, nodes_for

from sdirt_amd.basics import WAVE_RGB
from sdirt_amd.render_psf import (PSFVolume, _RenderPsfVolumeScene, local_dp_psf_render, local_dp_psf_render_volume,
                                  volume_segment_tables)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23

# (B, C, H, W, ks | Dz, Gy, Gx)
CASES = [(1, 3, 5, 9, 21, 3, 2, 2),        # image smaller than the pad
         (1, 3, 1, 7, 5, 2, 2, 2),         # one row
         (1, 3, 37, 53, 11, 3, 4, 4),      # interior, several cells
         (2, 4, 17, 33, 11, 5, 3, 2),      # batch, C = 4
         (1, 1, 19, 35, 21, 2, 2, 2),      # C = 1, a 7-D volume of one channel
         (1, 3, 6, 7, 5, 3, 9, 11),        # more nodes than pixels
         (1, 3, 16, 24, 11, 1, 3, 3),      # Dz = 1
         (1, 3, 16, 24, 11, 3, 1, 1),      # Gy = Gx = 1
         (1, 3, 12, 16, 63, 3, 2, 2),      # largest ks
         (1, 4, 8, 12, 63, 2, 2, 2),       # largest LDS ask
         # the gradient in the volume keeps the achromatic chunking per channel (the channel is a grid dimension): 4
         # planes of ks 63 fit in its 64 KB of sums, so 5 planes are two chunks, 4 planes and a short one of 1, and the
         # pixels between planes 3 and 4 have their two planes in different chunks
         (1, 3, 8, 12, 63, 5, 2, 2)]
INTERIOR, CHUNKED = CASES[2], CASES[-1]
DEPTHS = ["random", "constant", "on_nodes", "outside"]

_CACHE = {}


def problem(case, kind, seed=0):
    """Operands and tables of one case, made once and shared, on the GPU (where the float64 restatement runs too)."""
    key = (case, kind, seed)
    if key not in _CACHE:
        b, c, h, w, ks, dz, gy, gx = case
        gen = torch.Generator().manual_seed(1000 * seed + ks + h)
        xn, yn, zn = nodes_for(dz, gy, gx, gen)
        mk = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32)
        img, vol, G = mk(b, c, h, w), mk(c, dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w)
        z = depth_map(kind, (b, h, w), zn, gen)
        img, vol, G, z, xn, yn, zn = (t.to(DEV) for t in (img, vol, G, z, xn, yn, zn))
        tables = volume_segment_tables(xn, yn, zn, z, h, w)
        _CACHE[key] = dict(img=img, vol=vol, G=G, z=z, nodes=(xn, yn, zn), tables=tables)
    return _CACHE[key]


def stage(p, ks, vol=None, img=None, G=None):
    """The scene Function on the tables themselves, every operand a leaf -> (out, d volume, d image, d fz)."""
    ix, fx, iy, fy, iz, fz = p["tables"]
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    v, im, f = leaf(p["vol"] if vol is None else vol), leaf(p["img"] if img is None else img), leaf(fz)
    out = _RenderPsfVolumeScene.apply(v, im, f, ks, ix, fx, iy, fy, iz)
    out.backward(p["G"] if G is None else G)
    return out.detach(), v.grad, im.grad, f.grad


def results(case, kind):
    """stage() of a problem, run once."""
    p = problem(case, kind)
    if "got" not in p:
        p["got"] = stage(p, case[4])
    return p["got"]


def check(tag, got, want, scale, n):
    got, want, scale = got.detach().cpu().double(), want.cpu().double(), scale.cpu().double()
    n = torch.as_tensor(n).cpu().double()
    ratio = (got - want).abs() / (n * EPS * scale).clamp_min(1e-300)
    print(f"{tag}: worst |kernel - float64| / (n 2^-23 sum|terms|) = {float(ratio.max()):.3f} (n up to {int(n.max())})")
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= n * EPS * scale).all()), (tag, float(ratio.max()))


@pytest.mark.parametrize("kind", DEPTHS)
@pytest.mark.parametrize("case", CASES)
def test_forward_and_the_three_gradients_against_the_float64_restatement(case, kind):
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, kind)
    img, vol, G, tables = p["img"], p["vol"], p["G"], p["tables"]
    gl, gr = G[:, :c], G[:, c:]
    out, dvol, dimg, dfz = results(case, kind)
    assert out.shape == (b, 2 * c, h, w) and dvol.shape == vol.shape == (c, dz, gy, gx, 2, ks, ks)
    assert dimg.shape == img.shape and dfz.shape == (b, h, w)
    check(f"{case} {kind} forward", out, torch.cat(render_volume_chroma_f64(img, vol, tables, ks), 1),
          torch.cat(render_volume_chroma_abs(img, vol, tables, ks), 1), 8 * ks * ks + 8)
    counts = node_pixel_counts(tables, (dz, gy, gx))[None, ..., None, None, None]
    check(f"{case} {kind} d volume", dvol, volume_grad_chroma_f64(img, vol.shape, tables, gl, gr, ks),
          volume_grad_chroma_abs(img, vol.shape, tables, gl, gr, ks), counts + 8)
    untouched = (counts == 0).expand(vol.shape)
    assert not dvol[untouched].any()                             # exactly 0, not small
    if dz * gy * gx > 8 * b * h * w:
        assert bool(untouched.any())
    want_img, want_fz = scene_grads_chroma_f64(img, vol, tables, gl, gr, ks)
    check(f"{case} {kind} d image", dimg, want_img, dimg_chroma_abs(img, vol, tables, gl, gr, ks),
          16 * ks * ks * fold_counts(h, w, ks).to(DEV) + 8)
    check(f"{case} {kind} d fz", dfz, want_fz, dfz_chroma_abs(img, vol, tables, gl, gr, ks), 16 * c * ks * ks + 8)
    if dz == 1:
        assert not dfz.any()                                     # the two planes are the same node: exactly 0
    else:
        assert float(dfz.abs().max()) > 0
    assert float(dvol.abs().max()) > 0 and float(dimg.abs().max()) > 0


@pytest.mark.parametrize("kind", DEPTHS)
@pytest.mark.parametrize("case", CASES)
def test_every_channel_has_the_bits_of_the_achromatic_kernels_at_one_channel(case, kind):
    """The chromatic forward, dV[c] and d image[:, c] against the existing entries called at C = 1 on that channel's
    slices: the same helpers in the same order give the same bits.  (d fz is a sum over the channels and has no
    counterpart in separate calls.)"""
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, kind)
    out, dvol, dimg, _ = results(case, kind)
    for k in range(c):
        G1 = torch.cat([p["G"][:, k:k + 1], p["G"][:, c + k:c + k + 1]], 1).contiguous()
        out1, dvol1, dimg1, _ = stage(p, ks, vol=p["vol"][k], img=p["img"][:, k:k + 1].contiguous(), G=G1)
        assert dvol1.shape == (dz, gy, gx, 2, ks, ks)
        assert torch.equal(out[:, k], out1[:, 0]) and torch.equal(out[:, c + k], out1[:, 1]), k
        assert torch.equal(dvol[k], dvol1), k
        assert torch.equal(dimg[:, k:k + 1], dimg1), k


@pytest.mark.parametrize("case", CASES)
def test_equal_channels_collapse_onto_the_achromatic_path(case):
    """A 7-D volume with all channels equal renders what the 6-D path renders from one channel of it, bit for bit; the
    sum over the channels of its dV is the achromatic dV within the achromatic bar (top of this file)."""
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, "random")
    one = p["vol"][0].contiguous()
    same = one.expand(c, *one.shape).contiguous()
    out, dvol, dimg, dfz = stage(p, ks, vol=same)
    out1, dvol1, dimg1, dfz1 = stage(p, ks, vol=one)
    assert torch.equal(out, out1) and torch.equal(dimg, dimg1)
    with torch.no_grad():
        assert torch.equal(out, local_dp_psf_render_volume(p["img"], same, *p["nodes"], p["z"], ks))
        assert torch.equal(out, local_dp_psf_render_volume(p["img"], one, *p["nodes"], p["z"], ks))
    gl, gr = p["G"][:, :c], p["G"][:, c:]
    n = c * node_pixel_counts(p["tables"], (dz, gy, gx))[..., None, None, None] + 8
    want = volume_grad_f64(p["img"], one.shape, p["tables"], gl, gr, ks)
    scale = volume_grad_abs(p["img"], one.shape, p["tables"], gl, gr, ks)
    check(f"{case} sum over channels of d volume", dvol.sum(0), want, scale, n)
    check(f"{case} achromatic d volume", dvol1, want, scale, n)


@pytest.mark.parametrize("tap", ["first", "last"])
@pytest.mark.parametrize("side", [0, 1])
def test_a_one_hot_channel_reaches_its_own_channel_and_side_only(side, tap):
    """The volume is 0 except for one tap of one side of one node in channel k: every other output channel and the
    other side are exactly 0; channel k is w(pixel) img[k] at the flipped offset (within 8 2^-23 relative)."""
    b, c, h, w, ks, dz, gy, gx = INTERIOR
    p = problem(INTERIOR, "random")
    pad = (ks - 1) // 2
    i = j = 0 if tap == "first" else ks - 1
    P = torch.nn.functional.pad(p["img"].double(), (pad,) * 4, mode="replicate")
    shifted = P[:, :, ks - 1 - i:ks - 1 - i + h, ks - 1 - j:ks - 1 - j + w]
    for k in (0, c - 1):
        for node in [(0, 0, 0), (2, 1, 3), (dz - 1, gy - 1, gx - 1)]:
            vol = torch.zeros((c, dz, gy, gx, 2, ks, ks), device=DEV)
            vol[k][node][side, i, j] = 1.0
            with torch.no_grad():
                out = local_dp_psf_render_volume(p["img"], vol, *p["nodes"], p["z"], ks).double()
            wt = interpolate_kernels(vol[k].double(), p["tables"])[..., side, i, j]     # [B,H,W]: the node's weight
            want = wt * shifted[:, k]
            mine = out[:, side * c + k]
            rest = torch.ones(2 * c, dtype=torch.bool)
            rest[side * c + k] = False
            assert not out[:, rest].any()
            assert not mine[wt == 0].any()
            assert bool(((mine - want).abs() <= 8 * EPS * want.abs()).all())
            assert 0 < int((wt != 0).sum()) < h * w                                     # the node reaches part of the image


def test_two_runs_are_bit_identical_and_the_forward_under_grad_is_the_plain_forward():
    for case in [CASES[0], CASES[3], CASES[5], CHUNKED]:
        p = problem(case, "random")
        ks = case[4]
        first, second = stage(p, ks), stage(p, ks)
        for a, b in zip(first, second):
            assert torch.equal(a, b)
        with torch.no_grad():
            plain = local_dp_psf_render_volume(p["img"], p["vol"], *p["nodes"], p["z"], ks)
        assert torch.equal(first[0], plain)
        # the volume-only Function: same forward, same gradient
        v = p["vol"].detach().clone().requires_grad_(True)
        out = local_dp_psf_render_volume(p["img"], v, *p["nodes"], p["z"], ks)
        assert out.grad_fn is not None
        out.backward(p["G"])
        assert torch.equal(out.detach(), plain) and torch.equal(v.grad, first[1])
        # the public call with scene_grad=True: z.grad is d fz through torch's backward of axis_segments
        img, z = p["img"].clone().requires_grad_(True), p["z"].clone().requires_grad_(True)
        v = p["vol"].detach().clone().requires_grad_(True)
        out = local_dp_psf_render_volume(img, v, *p["nodes"], z, ks, scene_grad=True)
        out.backward(p["G"])
        assert torch.equal(out.detach(), plain) and torch.equal(v.grad, first[1]) and torch.equal(img.grad, first[2])
        assert z.grad.shape == p["z"].shape and bool(torch.isfinite(z.grad).all())


def test_an_empty_batch_through_the_three_entries():
    """B = 0: the forward and the scene gradients have nothing to write, the gradient in the volume still writes EVERY
    element, all 0.  All return SDIRT_OK."""
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    c, h, w, ks, dz, gy, gx = 3, 8, 9, 5, 3, 2, 2
    one = torch.zeros(4, device=DEV)
    ix, iy, iz = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (w, h, 1))
    fx, fy, fz = (torch.zeros(n, device=DEV) for n in (w, h, 1))
    vol = torch.rand((c, dz, gy, gx, 2, ks, ks), device=DEV)
    dvol = torch.full_like(vol, float("nan"))
    lib, st = _lib.lib(), stream_ptr(torch.device(DEV))
    tables = [dptr(t) for t in (ix, fx, iy, fy, iz, fz)]
    shape = (0, c, h, w, ks, dz, gy, gx)
    assert lib.sdirt_render_psf_volume_chroma(dptr(one), dptr(vol), *tables, *shape, dptr(one), dptr(one), st) == 0
    assert lib.sdirt_render_psf_volume_chroma_grad(dptr(one), dptr(one), dptr(one), *tables, *shape, dptr(dvol), st) == 0
    assert lib.sdirt_render_psf_volume_chroma_grad_scene(dptr(one), dptr(vol), dptr(one), dptr(one), *tables, *shape,
                                                         dptr(one), dptr(one), st) == 0
    torch.cuda.synchronize()
    assert not one.any() and not dvol.any() and bool(torch.isfinite(dvol).all())


def _pupil_of(lens, ks):
    torch.manual_seed(3)
    with torch.no_grad():
        lens.psf_lr(torch.tensor([[0.0, 0.0, -1500.0]]), ks=ks, spp=2048)
    return tuple(t.clone() for t in lens.last_pupil_points)


def test_psf_volume_with_the_three_wavelengths_is_three_volumes_stacked():
    lens = make_lens("rf50mm", DEV, load_state("rf50mm"))
    ks = 21
    pupil = _pupil_of(lens, ks)
    call = lambda **kw: lens.psf_volume(grid=(3, 3), z=2, ks=ks, spp=2048, pupil_xy=pupil[:2], center_pupil_xy=pupil[2:],
                                        **kw)
    with torch.no_grad():
        vol = call(wvln=WAVE_RGB)
        assert vol.psf.shape == (3, 2, 3, 3, 2, ks, ks) and vol.wvln == tuple(WAVE_RGB)
        for k, wave in enumerate(WAVE_RGB):
            single = call(wvln=wave)
            assert single.psf.shape == (2, 3, 3, 2, ks, ks) and single.wvln == (wave,)
            assert torch.equal(vol.psf[k], single.psf), wave
        assert torch.equal(vol.psf[1], call().psf)                   # green is the default wavelength
        # per-wavelength points in psf_rgb's convention [2, Cw, n]: the same sets three times are the shared call
        per = lens.psf_volume(grid=(3, 3), z=2, ks=ks, spp=2048, wvln=WAVE_RGB,
                              pupil_xy=torch.stack([torch.stack([t] * 3) for t in pupil[:2]]),
                              center_pupil_xy=torch.stack([torch.stack([t] * 3) for t in pupil[2:]]))
        assert torch.equal(per.psf, vol.psf)
    # lateral and axial colour: at the off-axis corner node the red and blue PSFs are not copies of the green one
    taps = torch.arange(ks, dtype=torch.float64, device=DEV)
    corner = vol.psf[:, 0, 0, 0].double()                            # [3, 2, ks, ks], each sum-normalised
    com = torch.stack(((corner.sum(-1) * taps).sum(-1), (corner.sum(-2) * taps).sum(-1)), -1)      # [3, 2 sides, (i, j)]
    print(f"centres of mass (row, column) at the corner node, L then R: red {com[0].tolist()}, green {com[1].tolist()}, "
          f"blue {com[2].tolist()}")
    assert bool((corner.sum((-1, -2)) > 0.5).all())
    assert not torch.equal(com[0], com[1]) and not torch.equal(com[2], com[1])
    assert not torch.equal(vol.psf[0], vol.psf[1]) and not torch.equal(vol.psf[2], vol.psf[1])


def _chain(lens, h_param, pupil, ks, render):
    vol = lens.psf_volume(grid=(3, 3), z=2, ks=ks, spp=2048, dp=(h_param, 1.44, 0.3, 0.5), wvln=WAVE_RGB,
                          pupil_xy=pupil[:2], center_pupil_xy=pupil[2:])
    return vol, render(vol)


def test_gradient_reaches_the_dp_sensor_through_a_chromatic_psf_volume_and_the_render():
    """The chain of test_gpu_render_volume.py's test of the same name with psf_volume(wvln=WAVE_RGB): the fused
    chromatic render of a 24 x 36 RGB image -> L2 loss against a shifted render.  h.grad must be finite, non-zero and
    within 2 max(s, 1e-4) relative of the composed path's (per channel: torch interpolation of that channel's volume +
    local_dp_psf_render), where s is the composed path's own spread: fp32 against the same graph with the render
    stage's gradient computed by the float64 restatement and passed back in (the rule of DESIGN.md sections 7d, 7f,
    7g).  One Adam step along the gradient lowers the loss; scene_grad=True reaches the depth and the image."""
    lens = make_lens("rf50mm", DEV, load_state("rf50mm"))
    H, W, ks, C = 24, 36, 21, 3
    pupil = _pupil_of(lens, ks)
    gen = torch.Generator().manual_seed(4)
    img = torch.rand((1, C, H, W), generator=gen).to(DEV)
    z = torch.rand((1, H, W), generator=gen).to(DEV)
    fused = lambda v: v.render(img, z)
    with torch.no_grad():                                  # the "captured" frame: another h, shifted by a pixel
        target = torch.roll(_chain(lens, 0.70, pupil, ks, fused)[1], 1, -1)
    loss_of = lambda out: ((out - target) ** 2).sum()

    h = torch.tensor(0.78, requires_grad=True)
    vol, out = _chain(lens, h, pupil, ks, fused)
    assert vol.psf.shape == (C, 2, 3, 3, 2, ks, ks) and vol.psf.grad_fn is not None
    loss = loss_of(out)
    loss.backward()
    g_fused = float(h.grad)

    def composed(v):
        tables = volume_segment_tables(v.x_nodes, v.y_nodes, v.z_nodes, z, H, W)
        per = [local_dp_psf_render(img[:, k:k + 1].contiguous(), interpolate_kernels(v.psf[k], tables), ks)
               for k in range(C)]
        return torch.cat([r[:, :1] for r in per] + [r[:, 1:] for r in per], 1)

    h2 = torch.tensor(0.78, requires_grad=True)
    vol2, out2 = _chain(lens, h2, pupil, ks, composed)
    # the same graph with the render stage's gradient from the float64 restatement
    tables = volume_segment_tables(vol2.x_nodes, vol2.y_nodes, vol2.z_nodes, z, H, W)
    v64 = vol2.psf.detach().cpu().double().requires_grad_(True)
    l64, r64 = render_volume_chroma_f64(img.cpu(), v64, tuple(t.cpu() for t in tables), ks)
    ((torch.cat([l64, r64], 1) - target.cpu().double()) ** 2).sum().backward()
    (g_f64,) = torch.autograd.grad(vol2.psf, h2, grad_outputs=v64.grad.float().to(DEV), retain_graph=True)
    loss_of(out2).backward()
    g_composed, g_f64 = float(h2.grad), float(g_f64)
    s = abs(g_composed - g_f64) / abs(g_f64)
    rel = abs(g_fused - g_composed) / abs(g_composed)
    print(f"d loss / d h: fused {g_fused:.9e}, composed {g_composed:.9e}, composed with the float64 render gradient "
          f"{g_f64:.9e}; spread s = {s:.3e}, |fused - composed| / |composed| = {rel:.3e}, allowed {2 * max(s, 1e-4):.3e}")
    assert np.isfinite(g_fused) and g_fused != 0.0
    assert rel <= 2 * max(s, 1e-4)
    opt = torch.optim.Adam([h], lr=0.005)
    opt.step()
    with torch.no_grad():
        _, after = _chain(lens, float(h.detach()), pupil, ks, fused)
    print(f"loss {float(loss.detach()):.6e} -> {float(loss_of(after)):.6e} after one Adam step "
          f"(h {0.78} -> {float(h.detach()):.4f})")
    assert float(loss_of(after)) < float(loss.detach())
    # the scene's gradients through the same chromatic volume (its values: the graph to h has been used)
    img_leaf, z_leaf = img.clone().requires_grad_(True), z.clone().requires_grad_(True)
    loss_of(dataclasses.replace(vol, psf=vol.psf.detach()).render(img_leaf, z_leaf, scene_grad=True)).backward()
    for name, g in (("z", z_leaf.grad), ("img", img_leaf.grad)):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name


def test_psfnet_render_volume_with_a_chromatic_volume_is_the_hand_composed_chain():
    from sdirt_amd.psfnet import PSFNet
    ks, H, W = 7, 20, 28
    net = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=ks, device=DEV,
                 post_computation=False)
    gen = torch.Generator().manual_seed(5)
    psf = torch.rand((3, 3, 2, 4, 2, ks, ks), generator=gen)
    psf = (psf / psf.sum((-1, -2), keepdim=True)).to(DEV)
    vol = PSFVolume(psf, torch.tensor([-0.75, -0.25, 0.25, 0.75]).to(DEV), torch.tensor([0.5, -0.5]).to(DEV),
                    torch.tensor([0.0, 0.05, 1.0]).to(DEV), net.d_min, net.d_max, tuple(WAVE_RGB))
    img = torch.rand((2, 3, H, W), generator=gen).to(DEV)
    depth = (-200.0 - 3000.0 * torch.rand((2, 1, H, W), generator=gen)).to(DEV)
    got = net.render_volume(img, depth, vol)
    z = net.depth2z(depth + net.d_sensor).squeeze(1)
    lin = local_dp_psf_render_volume(net.degamma(img), psf, vol.x_nodes, vol.y_nodes, vol.z_nodes, z, ks)
    assert torch.equal(got, torch.clip(net.gamma(lin), 0.0, 1.0))
    assert got.shape == (2, 6, H, W) and float(got.max()) > 0
    # the channels are rendered with different PSFs: not what the green volume alone gives
    assert not torch.equal(got, net.render_volume(img, depth, PSFVolume(psf[1], *[getattr(vol, n) for n in
                           ("x_nodes", "y_nodes", "z_nodes", "d_min", "d_max")])))
