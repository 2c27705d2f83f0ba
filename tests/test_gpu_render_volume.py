"""local_dp_psf_render_volume on the GPU: the two kernels of sdirt_render_volume.hip against the float64 restatement
(tests/render_volume_f64.py, which tests/test_render_volume_cpu.py holds against the reference's local_dp_psf_render,
grid_sample and numpy.interp).  The segment tables are computed once in fp32 and handed to both.

The bars are derived, not measured.  Unit 2^-23 (u = 2^-24 doubled, which covers the second-order terms):
  forward, per output element:  |kernel - float64| <= (8 ks^2 + 8) 2^-23 sum|terms|
      at most 5 roundings in a weight (three 1 - f, two products), 2 in the products with V and P, and at most
      8 ks^2 - 1 in the sum of the 8 ks^2 terms on any path through it;
  gradient, per dV element:     |kernel - float64| <= (n + 8) 2^-23 sum|terms|
      n = C x the number of (b, pixel) with a non-zero weight at the node: 5 roundings in a weight, 1 in w D, C products
      and C - 1 additions in D, and one addition per pixel.
sum|terms| is the same sum on the operands' magnitudes."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA, load_state, make_lens
from render_f64 import render_f64
from render_volume_f64 import (interpolate_kernels, node_pixel_counts, render_volume_abs, render_volume_f64,
                               sampled_dvol, sampled_out, volume_grad_abs, volume_grad_f64)

from sdirt_amd.render_psf import local_dp_psf_render, local_dp_psf_render_volume, volume_segment_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23

# (B, C, H, W, ks | Dz, Gy, Gx)
CASES = [(1, 3, 48, 80, 21, 4, 3, 5), (1, 3, 37, 53, 11, 3, 4, 4), (1, 3, 41, 50, 31, 2, 3, 2), (1, 3, 20, 27, 63, 2, 2, 3),
         (1, 1, 19, 35, 21, 2, 2, 2), (2, 4, 17, 33, 11, 5, 3, 2), (1, 3, 5, 9, 21, 3, 2, 2), (1, 3, 6, 7, 5, 3, 9, 11),
         (1, 3, 16, 24, 11, 1, 3, 3), (1, 3, 16, 24, 11, 3, 1, 1),
         # the backward's depth chunks: 4 planes of ks 63 fit in its 64 KB of sums, so 6 planes are two chunks, the last
         # one short, with pixels whose two planes lie in different chunks; the only case above 32 KB of dynamic LDS
         (1, 3, 12, 16, 63, 6, 2, 2)]
CHUNKED = CASES[-1]
DEPTHS = ["random", "constant", "on_nodes", "outside"]


def nodes_for(dz, gy, gx, gen):
    """Cell-centred x, DECREASING cell-centred y, NON-UNIFORM increasing z in [0, 1]."""
    x = torch.linspace(-1 + 1 / (2 * gx), 1 - 1 / (2 * gx), gx)
    y = torch.linspace(1 - 1 / (2 * gy), -1 + 1 / (2 * gy), gy)
    z = torch.cumsum(torch.rand(dz, generator=gen) + 0.05, 0)
    return x, y, (z - z[0]) / (z[-1] - z[0]) if dz > 1 else torch.tensor([0.4])


def depth_map(kind, shape, zn, gen):
    if kind == "random":                                   # every pixel in another segment
        return torch.rand(shape, generator=gen)
    if kind == "constant":
        return torch.full(shape, 0.37)
    if kind == "on_nodes":
        return zn[torch.randint(0, len(zn), shape, generator=gen)]
    return torch.rand(shape, generator=gen) * 2.0 - 0.5    # a quarter below the first node, a quarter above the last


_CACHE = {}


def problem(case, kind, seed=0):
    """Operands and tables of one case, made once and shared; they live on the GPU, where the float64 restatement runs
    as well (the ks 63 case takes a minute on the CPU)."""
    key = (case, kind, seed)
    if key not in _CACHE:
        b, c, h, w, ks, dz, gy, gx = case
        gen = torch.Generator().manual_seed(1000 * seed + ks + h)
        xn, yn, zn = nodes_for(dz, gy, gx, gen)
        mk = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32)
        img, vol, G = mk(b, c, h, w), mk(dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w)
        z = depth_map(kind, (b, h, w), zn, gen)
        img, vol, G, z, xn, yn, zn = (t.to(DEV) for t in (img, vol, G, z, xn, yn, zn))
        # the tables the kernel is handed: the ones the call under test makes from these operands
        tables = volume_segment_tables(xn, yn, zn, z, h, w)
        _CACHE[key] = dict(img=img, vol=vol, G=G, z=z, nodes=(xn, yn, zn), tables=tables)
    return _CACHE[key]


def run(p, ks, grad=True, G=None):
    vol = p["vol"].detach().clone().requires_grad_(grad)
    out = local_dp_psf_render_volume(p["img"], vol, *p["nodes"], p["z"], ks)
    if grad:
        assert out.grad_fn is not None
        out.backward(p["G"] if G is None else G)
    return out.detach(), vol.grad


def check(tag, got, want, scale, n):
    got, want, scale = got.detach().cpu().double(), want.cpu().double(), scale.cpu().double()
    n = torch.as_tensor(n).cpu().double()
    ratio = (got - want).abs() / (n * EPS * scale).clamp_min(1e-300)
    print(f"{tag}: worst |kernel - float64| / (n 2^-23 sum|terms|) = {float(ratio.max()):.3f} (n up to {int(n.max())})")
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= n * EPS * scale).all()), (tag, float(ratio.max()))


@pytest.mark.parametrize("kind", DEPTHS)
@pytest.mark.parametrize("case", CASES)
def test_forward_and_gradient_against_the_float64_restatement(case, kind):
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, kind)
    img, vol, G, tables = p["img"], p["vol"], p["G"], p["tables"]
    out, dvol = run(p, ks)
    assert out.shape == (b, 2 * c, h, w) and dvol.shape == vol.shape
    want = torch.cat(render_volume_f64(img, vol, tables, ks), 1)
    scale = torch.cat(render_volume_abs(img, vol, tables, ks), 1)
    check(f"{case} {kind} forward", out, want, scale, 8 * ks * ks + 8)
    gl, gr = G[:, :c], G[:, c:]
    counts = node_pixel_counts(tables, (dz, gy, gx))[..., None, None, None]
    check(f"{case} {kind} d volume", dvol, volume_grad_f64(img, vol.shape, tables, gl, gr, ks),
          volume_grad_abs(img, vol.shape, tables, gl, gr, ks), c * counts + 8)
    untouched = (counts == 0).expand(vol.shape)
    assert not dvol[untouched].any()                             # exactly 0, not small
    if dz * gy * gx > 8 * b * h * w:
        assert bool(untouched.any())
    assert float(dvol.abs().max()) > 0


@pytest.mark.parametrize("tap", ["first", "last"])
@pytest.mark.parametrize("side", [0, 1])
def test_one_hot_volumes_pin_the_order_the_flip_and_the_sides(side, tap):
    """One node holds a single 1 at the first or last tap of one side: the output is w(pixel) P at the flipped offset
    (within 8 2^-23 relative), exactly 0 on the other side and wherever the node's weight is 0."""
    case = (1, 3, 37, 53, 11, 3, 4, 4)
    b, c, h, w, ks, dz, gy, gx = case
    p = dict(problem(case, "random"))
    pad = (ks - 1) // 2
    i = j = 0 if tap == "first" else ks - 1
    P = torch.nn.functional.pad(p["img"].double(), (pad,) * 4, mode="replicate")
    shifted = P[:, :, ks - 1 - i:ks - 1 - i + h, ks - 1 - j:ks - 1 - j + w]
    for node in [(0, 0, 0), (2, 1, 3), (1, 3, 0), (dz - 1, gy - 1, gx - 1)]:
        vol = torch.zeros((dz, gy, gx, 2, ks, ks), device=DEV)
        vol[node][side, i, j] = 1.0
        p["vol"] = vol
        out, _ = run(p, ks, grad=False)
        out = out.double()
        wt = interpolate_kernels(vol.double(), p["tables"])[..., side, i, j]         # [B,H,W]: the node's weight
        want = wt[:, None] * shifted
        mine, other = out[:, side * c:(side + 1) * c], out[:, (1 - side) * c:(2 - side) * c]
        assert not other.any()
        assert not mine[(wt == 0)[:, None].expand_as(mine)].any()
        assert bool(((mine - want).abs() <= 8 * EPS * want.abs()).all())
        assert 0 < int((wt != 0).sum()) < h * w                                     # the node reaches part of the image


def test_a_volume_of_one_kernel_pair_renders_what_the_per_pixel_render_does():
    case = (1, 3, 37, 53, 11, 3, 4, 4)
    b, c, h, w, ks, dz, gy, gx = case
    p = dict(problem(case, "outside"))
    pair = torch.rand((2, ks, ks), generator=torch.Generator().manual_seed(3)).to(DEV)
    p["vol"] = pair.expand(dz, gy, gx, 2, ks, ks).contiguous()
    out, _ = run(p, ks, grad=False)
    per_pixel = local_dp_psf_render(p["img"], pair.expand(b, h, w, 2, ks, ks).contiguous(), ks)
    scale = torch.cat(render_volume_abs(p["img"], p["vol"], p["tables"], ks), 1)
    assert bool(((out - per_pixel).abs().double() <= (8 * ks * ks + 8) * EPS * scale).all())
    check("constant volume", out, torch.cat(render_volume_f64(p["img"], p["vol"], p["tables"], ks), 1), scale,
          8 * ks * ks + 8)


def test_forward_under_grad_is_bit_equal_and_two_runs_are_bit_identical():
    for case in [CASES[0], CASES[5], CASES[7], CHUNKED]:
        p = problem(case, "random")
        ks = case[4]
        out, dvol = run(p, ks)
        out2, dvol2 = run(p, ks)
        plain, none = run(p, ks, grad=False)
        assert none is None
        assert torch.equal(out, plain) and torch.equal(out, out2) and torch.equal(dvol, dvol2)


@pytest.mark.parametrize("side", [0, 1])
def test_upstream_zero_on_one_side_gives_that_side_exactly_zero(side):
    case = CASES[1]
    c, ks = case[1], case[4]
    p = problem(case, "random")
    G = p["G"].clone()
    G[:, side * c:(side + 1) * c] = 0
    _, dvol = run(p, ks, G=G)
    assert not dvol[:, :, :, side].any() and dvol[:, :, :, 1 - side].any()


def test_image_or_depth_requiring_a_gradient_is_refused():
    p = problem(CASES[6], "random")
    with pytest.raises(ValueError, match="image"):
        local_dp_psf_render_volume(p["img"].clone().requires_grad_(True), p["vol"], *p["nodes"], p["z"], 21)
    with pytest.raises(ValueError, match="depth"):
        local_dp_psf_render_volume(p["img"], p["vol"], *p["nodes"], p["z"].clone().requires_grad_(True), 21)
    with torch.no_grad():                                        # nothing is recorded: nothing is refused
        local_dp_psf_render_volume(p["img"].clone().requires_grad_(True), p["vol"], *p["nodes"], p["z"], 21)


@pytest.mark.parametrize("case", CASES[:3])
def test_volume_gradient_against_the_composed_path(case):
    """The kernels materialised with torch ops from the same tables, then local_dp_psf_render under autograd: the two
    fp32 gradients agree within the gradient bar."""
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, "random")
    _, dvol = run(p, ks)
    vol = p["vol"].detach().clone().requires_grad_(True)
    local_dp_psf_render(p["img"], interpolate_kernels(vol, p["tables"]), ks).backward(p["G"])
    gl, gr = p["G"][:, :c], p["G"][:, c:]
    n = c * node_pixel_counts(p["tables"], (dz, gy, gx))[..., None, None, None] + 8
    scale = volume_grad_abs(p["img"], vol.shape, p["tables"], gl, gr, ks)
    diff = (dvol - vol.grad).abs().double()
    print(f"{case}: worst |fused - composed| / bar = {float((diff / (n * EPS * scale).clamp_min(1e-300)).max()):.3f}")
    assert bool((diff <= n * EPS * scale).all())


def test_full_size_on_a_fixed_sample_of_outputs_and_gradients():
    """1 x 3 x 512 x 768, ks 21, volume 16 x 32 x 32: 256 output pixels and 256 dV elements drawn once from a seeded
    generator against the sampled float64 evaluators, same bars."""
    b, c, h, w, ks, dz, gy, gx = 1, 3, 512, 768, 21, 16, 32, 32
    gen = torch.Generator().manual_seed(12)
    xn, yn, zn = nodes_for(dz, gy, gx, gen)
    mk = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32).to(DEV)
    img, vol, G = mk(b, c, h, w), mk(dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w)
    z = (torch.rand((b, h, w), generator=gen) * 1.2 - 0.1).to(DEV)
    tables = volume_segment_tables(xn.to(DEV), yn.to(DEV), zn.to(DEV), z, h, w)
    v = vol.clone().requires_grad_(True)
    out = local_dp_psf_render_volume(img, v, xn.to(DEV), yn.to(DEV), zn.to(DEV), z, ks)
    out.backward(G)
    pick = lambda n: torch.randint(0, n, (256,), generator=gen)
    idx = torch.stack([pick(n) for n in (b, c, h, w)], 1).to(DEV)
    idx[:4, 2:] = torch.tensor([[0, 0], [0, w - 1], [h - 1, 0], [h - 1, w - 1]], device=DEV)      # the image's corners
    want, scale = sampled_out(img, vol, tables, ks, idx), sampled_out(img, vol, tables, ks, idx, absolute=True)
    bi, ci, yi, xi = idx.unbind(1)
    got = torch.stack((out[bi, ci, yi, xi], out[bi, ci + c, yi, xi]), 1)
    check("full size forward", got, want, scale, 8 * ks * ks + 8)
    idx = torch.stack([pick(n) for n in (dz, gy, gx, 2, ks, ks)], 1)
    idx[:4, :3] = torch.tensor([[0, 0, 0], [dz - 1, gy - 1, gx - 1], [0, gy - 1, 0], [dz - 1, 0, gx - 1]])
    gl, gr = G[:, :c], G[:, c:]
    want, n = sampled_dvol(img, gl, gr, tables, (dz, gy, gx), ks, idx)
    scale, _ = sampled_dvol(img, gl, gr, tables, (dz, gy, gx), ks, idx, absolute=True)
    check("full size d volume", v.grad[tuple(idx.to(DEV).unbind(1))], want, scale, c * n + 8)
    assert int(n.max()) > 0


def _chain(lens, h_param, pupil, img, z, ks, render):
    vol = lens.psf_volume(grid=(3, 3), z=2, ks=ks, spp=2048, dp=(h_param, 1.44, 0.3, 0.5), pupil_xy=pupil[:2],
                          center_pupil_xy=pupil[2:])
    return vol, render(vol)


def test_gradient_reaches_the_dp_sensor_through_psf_volume_and_the_render():
    """make_lens -> psf_volume(grid 3 x 3, 2 depths, ks 21, spp 2048, h requiring grad, fixed pupil points) -> the
    fused render of a 24 x 36 image -> L2 loss against a shifted render.  h.grad must be finite, non-zero and within
    2 max(s, 1e-4) relative of the composed path's (torch interpolation + local_dp_psf_render), where s is the composed
    path's own spread: fp32 local_dp_psf_render against the same graph with the render stage's gradient computed by the
    float64 restatement and passed back in (the rule of DESIGN.md sections 7d, 7f).  Measured on an MI355X: see
    DESIGN.md section 7g.  One Adam step along the gradient lowers the loss."""
    lens = make_lens("rf50mm", DEV, load_state("rf50mm"))
    H, W, ks, C = 24, 36, 21, 3
    torch.manual_seed(3)
    with torch.no_grad():
        lens.psf_lr(torch.tensor([[0.0, 0.0, -1500.0]]), ks=ks, spp=2048)
    pupil = tuple(t.clone() for t in lens.last_pupil_points)
    gen = torch.Generator().manual_seed(4)
    img = torch.rand((1, C, H, W), generator=gen).to(DEV)
    z = torch.rand((1, H, W), generator=gen).to(DEV)
    fused = lambda v: v.render(img, z)
    with torch.no_grad():                                  # the "captured" frame: another h, shifted by a pixel
        target = torch.roll(_chain(lens, 0.70, pupil, img, z, ks, fused)[1], 1, -1)
    loss_of = lambda out: ((out - target) ** 2).sum()

    h = torch.tensor(0.78, requires_grad=True)
    vol, out = _chain(lens, h, pupil, img, z, ks, fused)
    assert vol.psf.shape == (2, 3, 3, 2, ks, ks) and vol.psf.grad_fn is not None
    loss = loss_of(out)
    loss.backward()
    g_fused = float(h.grad)

    def composed(v):
        tables = volume_segment_tables(v.x_nodes, v.y_nodes, v.z_nodes, z, H, W)
        return local_dp_psf_render(img, interpolate_kernels(v.psf, tables), ks)

    h2 = torch.tensor(0.78, requires_grad=True)
    vol2, out2 = _chain(lens, h2, pupil, img, z, ks, composed)
    # the same graph with the render stage's gradient from the float64 restatement
    tables = volume_segment_tables(vol2.x_nodes, vol2.y_nodes, vol2.z_nodes, z, H, W)
    v64 = vol2.psf.detach().cpu().double().requires_grad_(True)
    l64, r64 = render_volume_f64(img.cpu(), v64, tuple(t.cpu() for t in tables), ks)
    ((torch.cat([l64, r64], 1) - target.cpu().double()) ** 2).sum().backward()
    (g_f64,) = torch.autograd.grad(vol2.psf, h2, grad_outputs=v64.grad.float().to(DEV), retain_graph=True)
    vol2.psf.retain_grad()
    loss_of(out2).backward()
    # the two graphs differ where they should: the render stage's fp32 gradient is not the rounded float64 one
    g32, g64 = vol2.psf.grad, v64.grad.float().to(DEV)
    differing = int((g32 != g64).sum())
    print(f"render-stage gradient in the volume: {differing} of {g32.numel()} elements differ between fp32 and rounded "
          f"float64, worst relative difference {float(((g32 - g64).abs() / g64.abs().clamp_min(1e-30)).max()):.3e}")
    assert differing > 0
    g_composed, g_f64 = float(h2.grad), float(g_f64)
    print(f"d loss / d h to 17 digits: composed {h2.grad.double().item():.17e}, with the float64 render gradient "
          f"{g_f64:.17e}")
    s = abs(g_composed - g_f64) / abs(g_f64)
    rel = abs(g_fused - g_composed) / abs(g_composed)
    print(f"d loss / d h: fused {g_fused:.9e}, composed {g_composed:.9e}, composed with the float64 render gradient "
          f"{g_f64:.9e}; spread s = {s:.3e}, |fused - composed| / |composed| = {rel:.3e}, allowed {2 * max(s, 1e-4):.3e}")
    assert np.isfinite(g_fused) and g_fused != 0.0
    assert rel <= 2 * max(s, 1e-4)
    opt = torch.optim.Adam([h], lr=0.005)
    opt.step()
    with torch.no_grad():
        _, after = _chain(lens, float(h), pupil, img, z, ks, fused)
    print(f"loss {float(loss.detach()):.6e} -> {float(loss_of(after)):.6e} after one Adam step (h {0.78} -> {float(h):.4f})")
    assert float(loss_of(after)) < float(loss.detach())


def test_psfnet_render_volume_is_the_hand_composed_chain():
    from sdirt_amd.psfnet import PSFNet
    from sdirt_amd.render_psf import PSFVolume
    ks, H, W = 7, 20, 28
    net = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=ks, device=DEV,
                 post_computation=False)
    gen = torch.Generator().manual_seed(5)
    psf = torch.rand((3, 2, 4, 2, ks, ks), generator=gen)
    psf = (psf / psf.sum((-1, -2), keepdim=True)).to(DEV)
    vol = PSFVolume(psf, torch.tensor([-0.75, -0.25, 0.25, 0.75]).to(DEV), torch.tensor([0.5, -0.5]).to(DEV),
                    torch.tensor([0.0, 0.05, 1.0]).to(DEV), net.d_min, net.d_max)
    img = torch.rand((2, 3, H, W), generator=gen).to(DEV)
    depth = (-200.0 - 3000.0 * torch.rand((2, 1, H, W), generator=gen)).to(DEV)
    got = net.render_volume(img, depth, vol)
    z = net.depth2z(depth + net.d_sensor).squeeze(1)
    lin = local_dp_psf_render_volume(net.degamma(img), psf, vol.x_nodes, vol.y_nodes, vol.z_nodes, z, ks)
    assert torch.equal(got, torch.clip(net.gamma(lin), 0.0, 1.0))
    assert got.shape == (2, 6, H, W) and float(got.max()) > 0
    torch.manual_seed(6)
    np.random.seed(6)
    noisy = net.render_volume(img, depth, vol, train=True)
    assert noisy.shape == got.shape and not torch.equal(noisy, got)


def test_an_empty_batch_renders_nothing_and_gives_a_zero_gradient():
    """B = 0 through the C entries: the forward has no element to write, the backward still writes EVERY element of
    grad_volume, all 0.  Both return SDIRT_OK."""
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    c, h, w, ks, dz, gy, gx = 3, 8, 9, 5, 3, 2, 2
    one = torch.zeros(4, device=DEV)
    ix, iy, iz = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (w, h, 1))
    fx, fy, fz = (torch.zeros(n, device=DEV) for n in (w, h, 1))
    vol = torch.rand((dz, gy, gx, 2, ks, ks), device=DEV)
    dvol = torch.full_like(vol, float("nan"))
    lib, st = _lib.lib(), stream_ptr(torch.device(DEV))
    tables = [dptr(t) for t in (ix, fx, iy, fy, iz, fz)]
    assert lib.sdirt_render_psf_volume(dptr(one), dptr(vol), *tables, 0, c, h, w, ks, dz, gy, gx, dptr(one), dptr(one), st) == 0
    assert lib.sdirt_render_psf_volume_grad(dptr(one), dptr(one), dptr(one), *tables, 0, c, h, w, ks, dz, gy, gx,
                                            dptr(dvol), st) == 0
    torch.cuda.synchronize()
    assert not one.any() and not dvol.any() and bool(torch.isfinite(dvol).all())
