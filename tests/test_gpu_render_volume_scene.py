"""local_dp_psf_render_volume(..., scene_grad=True) on the GPU: k_render_psf_volume_grad_img and
k_render_psf_volume_grad_depth against the float64 restatement (tests/render_volume_scene_f64.py, which
tests/test_render_volume_scene_cpu.py holds against central differences and grid_sample's autograd).  The segment tables
are computed once in fp32 and handed to both.

The bars are derived, not measured, and bind no summation order.  Unit 2^-23 (u = 2^-24 doubled, which covers the
second-order terms); sum|terms| is the same sum on the operands' magnitudes:
  d image, per element:  |kernel - float64| <= (16 ks^2 m + 8) 2^-23 sum|terms|
      m = the padded positions that clamp onto the element (1 inside, up to (pad + 1)^2 at a corner): 2 * 8 * ks^2 * m
      terms, each with at most 5 roundings in the weight and 2 in the products;
  d fz, per pixel:       |kernel - float64| <= (16 C ks^2 + 8) 2^-23 sum|terms|
      2 * C * 8 * ks^2 terms, each with at most 3 roundings in the weight and 3 in the products.
The step from fz to z is torch's autograd through axis_segments and is checked as such."""
import os

import pytest
import torch

from conftest import DATA
from render_volume_f64 import interpolate_kernels, render_volume_f64
from render_volume_scene_f64 import (dfz_abs, dimg_abs, fold_counts, sampled_dfz, sampled_dimg, scene_grads_f64)
from test_gpu_render_volume import depth_map, nodes_for

from sdirt_amd.render_psf import (_RenderPsfVolumeScene, axis_segments, local_dp_psf_render,
                                  local_dp_psf_render_volume, volume_segment_tables)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23

# (B, C, H, W, ks | Dz, Gy, Gx)
CASES = [(1, 3, 5, 9, 21, 3, 2, 2),        # image smaller than pad: every position is border, both clamps overlap
         (1, 3, 1, 7, 5, 2, 2, 2),         # one row: both ends fold onto the same row
         (1, 3, 37, 53, 11, 3, 4, 4),      # interior, several cells
         (2, 4, 17, 33, 11, 5, 3, 2),      # batch, C = 4
         (1, 1, 19, 35, 21, 2, 2, 2),      # C = 1
         (1, 3, 12, 16, 63, 2, 2, 2),      # largest ks, longest folds
         (1, 3, 16, 24, 11, 1, 3, 3),      # Dz = 1
         (1, 3, 6, 7, 5, 3, 9, 11)]        # more nodes than pixels
INTERIOR = CASES[2]
DEPTHS = ["random", "constant", "on_nodes", "outside"]

_CACHE = {}


def problem(case, kind, seed=0):
    """Operands, tables and the float64 gradients of one case, made once and shared (all on the GPU, where the float64
    restatement runs as well)."""
    key = (case, kind, seed)
    if key not in _CACHE:
        b, c, h, w, ks, dz, gy, gx = case
        gen = torch.Generator().manual_seed(1000 * seed + ks + h)
        xn, yn, zn = nodes_for(dz, gy, gx, gen)
        mk = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32)
        img, vol, G = mk(b, c, h, w), mk(dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w)
        z = depth_map(kind, (b, h, w), zn, gen)
        img, vol, G, z, xn, yn, zn = (t.to(DEV) for t in (img, vol, G, z, xn, yn, zn))
        tables = volume_segment_tables(xn, yn, zn, z, h, w)
        _CACHE[key] = dict(img=img, vol=vol, G=G, z=z, nodes=(xn, yn, zn), tables=tables)
    return _CACHE[key]


def reference(case, kind):
    """(d img, d fz, sum|terms| of d img, sum|terms| of d fz) in float64, computed once per problem."""
    p = problem(case, kind)
    if "ref" not in p:
        c, ks = case[1], case[4]
        gl, gr = p["G"][:, :c], p["G"][:, c:]
        dimg, dfz = scene_grads_f64(p["img"], p["vol"], p["tables"], gl, gr, ks)
        p["ref"] = (dimg, dfz, dimg_abs(p["img"], p["vol"], p["tables"], gl, gr, ks),
                    dfz_abs(p["img"], p["vol"], p["tables"], gl, gr, ks))
    return p["ref"]


def run(p, ks, G=None, vol=None, leaves=(True, True, True)):
    """The public call with scene_grad=True and (image, depth, volume) leaves -> (out, img.grad, z.grad, vol.grad)."""
    leaf = lambda t, on: t.detach().clone().requires_grad_(on)
    img, z, v = leaf(p["img"], leaves[0]), leaf(p["z"], leaves[1]), leaf(p["vol"] if vol is None else vol, leaves[2])
    out = local_dp_psf_render_volume(img, v, *p["nodes"], z, ks, scene_grad=True)
    assert out.grad_fn is not None
    out.backward(p["G"] if G is None else G)
    return out.detach(), img.grad, z.grad, v.grad


def stage(p, ks, G=None, vol=None):
    """The Function on the tables themselves -> (d img, d fz): the kernel's gradient in the TABLE VALUE."""
    ix, fx, iy, fy, iz, fz = p["tables"]
    img, fz = p["img"].detach().clone().requires_grad_(True), fz.detach().clone().requires_grad_(True)
    out = _RenderPsfVolumeScene.apply(p["vol"] if vol is None else vol, img, fz, ks, ix, fx, iy, fy, iz)
    out.backward(p["G"] if G is None else G)
    return img.grad, fz.grad


def check(tag, got, want, scale, n):
    got, want, scale = got.detach().cpu().double(), want.cpu().double(), scale.cpu().double()
    n = torch.as_tensor(n).cpu().double()
    ratio = (got - want).abs() / (n * EPS * scale).clamp_min(1e-300)
    print(f"{tag}: worst |kernel - float64| / (n 2^-23 sum|terms|) = {float(ratio.max()):.3f} (n up to {int(n.max())})")
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= n * EPS * scale).all()), (tag, float(ratio.max()))


def z_from_fz(p, dfz):
    """What torch's autograd through axis_segments makes of a gradient in fz -> (d z, the segment slope d fz / d z)."""
    z = p["z"].detach().clone().requires_grad_(True)
    fz = axis_segments(p["nodes"][2], z)[1]
    if not fz.requires_grad:                                     # an axis of one node: fz does not depend on z
        return torch.zeros_like(z), torch.zeros_like(z)
    assert torch.equal(fz.detach(), p["tables"][5])
    (dz,) = torch.autograd.grad(fz, z, grad_outputs=dfz, retain_graph=True)
    (slope,) = torch.autograd.grad(fz.sum(), z)
    return dz, slope


@pytest.mark.parametrize("kind", DEPTHS)
@pytest.mark.parametrize("case", CASES)
def test_scene_gradients_against_the_float64_restatement(case, kind):
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, kind)
    out, dimg, dzz, dvol = run(p, ks)
    assert dimg.shape == p["img"].shape and dimg.dtype == torch.float32 and dzz.shape == p["z"].shape
    # the forward is the plain call's, the volume's gradient the existing path's, bit for bit
    v = p["vol"].detach().clone().requires_grad_(True)
    plain = local_dp_psf_render_volume(p["img"], v, *p["nodes"], p["z"], ks)
    plain.backward(p["G"])
    with torch.no_grad():
        assert torch.equal(out, local_dp_psf_render_volume(p["img"], p["vol"], *p["nodes"], p["z"], ks))
    assert torch.equal(out, plain.detach()) and torch.equal(dvol, v.grad)
    # the stage on the tables: the same image gradient, and the gradient in fz that z.grad is made of
    dimg2, dfz = stage(p, ks)
    assert torch.equal(dimg, dimg2)
    want_img, want_fz, scale_img, scale_fz = reference(case, kind)
    m = fold_counts(h, w, ks).to(DEV)
    check(f"{case} {kind} d image", dimg, want_img, scale_img, 16 * ks * ks * m + 8)
    check(f"{case} {kind} d fz", dfz, want_fz, scale_fz, 16 * c * ks * ks + 8)
    # z.grad is the fz gradient through torch's own backward of axis_segments: the segment's slope, 0 outside the nodes
    want_z, slope = z_from_fz(p, dfz)
    assert torch.equal(dzz, want_z)
    assert bool(((dzz - dfz * slope).abs() <= 2 * EPS * (dfz * slope).abs()).all())
    zn = p["nodes"][2]
    outside = (p["z"] < zn.min()) | (p["z"] > zn.max())
    assert not dzz[outside].any() and not slope[outside].any()
    if kind == "outside":
        assert int(outside.sum()) > 0
    if dz == 1:
        assert not dfz.any() and not dzz.any()
    else:
        assert float(dfz.abs().max()) > 0 and (kind == "outside" or float(dzz.abs().max()) > 0)
        assert bool((slope[~outside] != 0).all())                # on the nodes too, the end nodes included
    assert float(dimg.abs().max()) > 0


def test_two_runs_are_bit_identical_and_only_what_is_asked_for_is_computed():
    for case in [CASES[0], CASES[3], CASES[5], CASES[7]]:
        p = problem(case, "random")
        ks = case[4]
        first, second = run(p, ks), run(p, ks)
        for a, b in zip(first, second):
            assert torch.equal(a, b)
        for leaves in [(True, False, False), (False, True, False), (False, False, True), (True, True, False)]:
            out, dimg, dzz, dvol = run(p, ks, leaves=leaves)
            assert torch.equal(out, first[0])
            for got, ref, on in zip((dimg, dzz, dvol), first[1:], leaves):
                assert (got is None) if not on else torch.equal(got, ref)


@pytest.mark.parametrize("side", [0, 1])
def test_upstream_zero_on_one_side_makes_that_side_of_the_volume_irrelevant(side):
    """G = 0 on one side: every term of that side is 0 * finite, so the image and fz gradients do not change by a bit
    when that side of the volume is replaced; they do change with the other side."""
    case = INTERIOR
    c, ks = case[1], case[4]
    p = problem(case, "random")
    G = p["G"].clone()
    G[:, side * c:(side + 1) * c] = 0
    dimg, dfz = stage(p, ks, G=G)
    other = torch.randn(p["vol"].shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    swapped = p["vol"].clone()
    swapped[:, :, :, side] = other[:, :, :, side]
    dimg2, dfz2 = stage(p, ks, G=G, vol=swapped)
    assert torch.equal(dimg, dimg2) and torch.equal(dfz, dfz2) and dimg.any() and dfz.any()
    swapped = p["vol"].clone()
    swapped[:, :, :, 1 - side] = other[:, :, :, 1 - side]
    dimg3, dfz3 = stage(p, ks, G=G, vol=swapped)
    assert not torch.equal(dimg, dimg3) and not torch.equal(dfz, dfz3)
    gl, gr = G[:, :c], G[:, c:]
    check(f"G_{'lr'[side]} = 0, d image", dimg, scene_grads_f64(p["img"], p["vol"], p["tables"], gl, gr, ks)[0],
          dimg_abs(p["img"], p["vol"], p["tables"], gl, gr, ks), 16 * ks * ks * fold_counts(*case[2:5]).to(DEV) + 8)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("corner", ["first", "last"])
def test_one_hot_upstream_at_a_corner_pixel_gives_its_flipped_kernel_folded_onto_the_border(corner, side):
    """G is a single 1 (one side, one channel) at a corner pixel of the image: d image of that channel is that
    pixel's interpolated kernel at the flipped offsets, with every tap that reads the padding folded onto the border,
    within 8 2^-23 relative; every other element is exactly 0, and so is d fz at every other pixel.  The volume is not
    negative here, so that `relative` has a meaning (no cancellation in the kernel or in the fold)."""
    case = INTERIOR
    b, c, h, w, ks, dz, gy, gx = case
    pad = (ks - 1) // 2
    p = dict(problem(case, "random"))
    p["vol"] = torch.rand(p["vol"].shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    y, x = (0, 0) if corner == "first" else (h - 1, w - 1)
    ch = 1
    G = torch.zeros_like(p["G"])
    G[0, side * c + ch, y, x] = 1.0
    dimg, dfz = stage(p, ks, G=G)
    K = interpolate_kernels(p["vol"].double(), p["tables"])[0, y, x, side]          # [ks,ks] float64
    want = torch.zeros((h, w), dtype=torch.float64, device=DEV)
    for i in range(ks):
        for j in range(ks):
            want[min(max(y + pad - i, 0), h - 1), min(max(x + pad - j, 0), w - 1)] += K[i, j]
    got = dimg[0, ch].double()
    ratio = ((got - want).abs() / (EPS * want.abs()).clamp_min(1e-300)).max()
    print(f"one-hot G at {corner} corner, side {side}: worst |kernel - float64| / (2^-23 |value|) = {float(ratio):.3f}")
    assert bool(((got - want).abs() <= 8 * EPS * want.abs()).all())
    assert int((want != 0).sum()) == (pad + 1) ** 2 and not got[want == 0].any()
    assert not dimg[0, [k for k in range(c) if k != ch]].any()
    assert float(dfz[0, y, x]) != 0.0
    dfz[0, y, x] = 0.0
    assert not dfz.any()


@pytest.mark.parametrize("case", CASES[:3])
def test_image_gradient_against_the_composed_path(case):
    """The kernels materialised with torch ops from the same tables, then local_dp_psf_render under autograd: the two
    fp32 image gradients agree within the bar."""
    b, c, h, w, ks, dz, gy, gx = case
    p = problem(case, "random")
    dimg, _ = stage(p, ks)
    img = p["img"].detach().clone().requires_grad_(True)
    local_dp_psf_render(img, interpolate_kernels(p["vol"], p["tables"]), ks).backward(p["G"])
    n = 16 * ks * ks * fold_counts(h, w, ks).to(DEV) + 8
    scale = reference(case, "random")[2]
    diff = (dimg - img.grad).abs().double()
    print(f"{case}: worst |fused - composed| / bar = {float((diff / (n * EPS * scale).clamp_min(1e-300)).max()):.3f}")
    assert bool((diff <= n * EPS * scale).all())


def test_full_size_on_a_fixed_sample_of_both_gradients():
    """1 x 3 x 512 x 768, ks 21, volume 16 x 32 x 32: 256 d image elements (the four corners and edge positions among
    them) and 256 d fz pixels drawn once from a seeded generator against the sampled float64 evaluators, same bars."""
    b, c, h, w, ks, dz, gy, gx = 1, 3, 512, 768, 21, 16, 32, 32
    gen = torch.Generator().manual_seed(12)
    xn, yn, zn = (t.to(DEV) for t in nodes_for(dz, gy, gx, gen))
    mk = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32).to(DEV)
    img, vol, G = mk(b, c, h, w), mk(dz, gy, gx, 2, ks, ks), mk(b, 2 * c, h, w)
    z = (torch.rand((b, h, w), generator=gen) * 1.2 - 0.1).to(DEV)
    tables = volume_segment_tables(xn, yn, zn, z, h, w)
    p = dict(img=img, vol=vol, G=G, z=z, nodes=(xn, yn, zn), tables=tables)
    dimg, dfz = stage(p, ks)
    gl, gr = G[:, :c], G[:, c:]
    pick = lambda n: torch.randint(0, n, (256,), generator=gen)
    idx = torch.stack([pick(n) for n in (b, c, h, w)], 1)
    idx[:4, 2:] = torch.tensor([[0, 0], [0, w - 1], [h - 1, 0], [h - 1, w - 1]])                # the image's corners
    idx[4:12, 2] = torch.tensor([0, 0, h - 1, h - 1, 1, h - 2, 9, 10])                          # edges and next to them
    idx[12:20, 3] = torch.tensor([0, 0, w - 1, w - 1, 1, w - 2, 9, 10])
    want = sampled_dimg(vol, gl, gr, tables, ks, idx)
    scale = sampled_dimg(vol, gl, gr, tables, ks, idx, absolute=True)
    m = fold_counts(h, w, ks)[idx[:, 2], idx[:, 3]]
    check("full size d image", dimg[tuple(idx.to(DEV).unbind(1))], want, scale, 16 * ks * ks * m + 8)
    assert int(m.max()) == 121
    idx = torch.stack([pick(n) for n in (b, h, w)], 1).to(DEV)
    idx[:4, 1:] = torch.tensor([[0, 0], [0, w - 1], [h - 1, 0], [h - 1, w - 1]], device=DEV)
    want = sampled_dfz(img, vol, gl, gr, tables, ks, idx)
    scale = sampled_dfz(img, vol, gl, gr, tables, ks, idx, absolute=True)
    check("full size d fz", dfz[tuple(idx.unbind(1))], want, scale, 16 * c * ks * ks + 8)
    assert float(dfz.abs().max()) > 0


def test_an_empty_batch_writes_nothing():
    from sdirt_amd import _lib
    from sdirt_amd.basics import dptr, stream_ptr
    c, h, w, ks, dz, gy, gx = 3, 8, 9, 5, 3, 2, 2
    one = torch.zeros(4, device=DEV)
    ix, iy, iz = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (w, h, 1))
    fx, fy, fz = (torch.zeros(n, device=DEV) for n in (w, h, 1))
    vol = torch.rand((dz, gy, gx, 2, ks, ks), device=DEV)
    tables = [dptr(t) for t in (ix, fx, iy, fy, iz, fz)]
    rc = _lib.lib().sdirt_render_psf_volume_grad_scene(dptr(one), dptr(vol), dptr(one), dptr(one), *tables, 0, c, h, w, ks,
                                                       dz, gy, gx, dptr(one), dptr(one), stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0 and not one.any()


class _RenderStageF64(torch.autograd.Function):
    """The render stage of the chain with the float64 restatement's output and gradients (rounded to fp32 where they
    re-enter the fp32 graph); keeps the upstream gradient it was handed."""

    @staticmethod
    def forward(ctx, img, fz, vol, tables, ks, seen):
        ctx.save_for_backward(img, fz)
        ctx.rest = (vol, tables, ks, seen)
        left, right = render_volume_f64(img, vol, (*tables[:5], fz), ks)
        return torch.cat([left, right], 1).float()

    @staticmethod
    def backward(ctx, grad):
        img, fz = ctx.saved_tensors
        vol, tables, ks, seen = ctx.rest
        c = img.shape[1]
        seen["G"] = grad.detach().clone()
        with torch.enable_grad():
            dimg, dfz = scene_grads_f64(img, vol, (*tables[:5], fz), grad[:, :c], grad[:, c:], ks)
        return dimg.float(), dfz.float(), None, None, None, None


def test_depth_and_image_gradients_through_psfnet_render_volume():
    """rf50mm, psf_volume(grid 3 x 3, 4 depths, ks 11, spp 1024), a 24 x 32 image, the depth a tilted plane inside
    [d_min, d_max]; PSFNet.render_volume(img, depth, vol, scene_grad=True) -> L2 loss against the render of another
    plane -> depth.grad, img.grad, against the same graph with the render stage replaced by a stub Function that returns
    the float64 restatement's output and gradients.  Allowed per element: the stage's bar (top of this file, on the
    upstream gradient the stub was handed) times the torch-side multiplier |d fz / d depth| (for the image: |degamma'|),
    each from autograd of the torch ops alone, plus 4 2^-23 |value| for the torch ops' own fp32 roundings.  (The two
    graphs hand the stage upstream gradients that differ by the forward's rounding, about 2^-23 of an output value
    against a residual of 1e-2 of it and more: two to three orders below the bar.)  Then, printed and asserted only as
    loss_after < loss_before: a few Adam steps on the depth, from the perturbed plane, lower the loss."""
    from sdirt_amd.psfnet import PSFNet
    ks, H, W, C = 11, 24, 32, 3
    net = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=ks, device=DEV)
    net.refocus(-1000 + net.d_sensor)
    torch.manual_seed(3)
    with torch.no_grad():
        vol = net.psf_volume(grid=(3, 3), z=4, ks=ks, spp=1024)
    assert vol.psf.shape == (4, 3, 3, 2, ks, ks) and not vol.psf.requires_grad
    gen = torch.Generator().manual_seed(4)
    img0 = (0.1 + 0.8 * torch.rand((1, C, H, W), generator=gen)).to(DEV)
    ramp = torch.linspace(0, 1, W).reshape(1, 1, 1, W) * 0.7 + torch.linspace(0, 1, H).reshape(1, 1, H, 1) * 0.3
    true_depth = (-1000.0 - 14000.0 * ramp).to(DEV) - net.d_sensor            # a tilted plane, 1 m ... 15 m
    start = (-1300.0 - 15500.0 * ramp.flip(-2)).to(DEV) - net.d_sensor        # another plane, tilted the other way in y
    assert net.d_max < float(start.min()) + net.d_sensor and float(true_depth.max()) + net.d_sensor < net.d_min
    with torch.no_grad():
        target = net.render_volume(img0, true_depth, vol)
    loss_of = lambda out: ((out - target) ** 2).sum()

    img, depth = img0.clone().requires_grad_(True), start.clone().requires_grad_(True)
    loss_of(net.render_volume(img, depth, vol, scene_grad=True)).backward()

    # the same graph, the render stage from the float64 restatement
    img2, depth2 = img0.clone().requires_grad_(True), start.clone().requires_grad_(True)
    z = net.depth2z(depth2 + net.d_sensor).squeeze(1)
    tables = volume_segment_tables(vol.x_nodes, vol.y_nodes, vol.z_nodes, z.detach(), H, W)
    fz = axis_segments(vol.z_nodes, z)[1]
    lin = net.degamma(img2)
    assert torch.equal(fz.detach(), tables[5])
    seen = {}
    # the torch-side multipliers, by autograd of the torch ops alone (both are elementwise)
    (dfz_ddepth,) = torch.autograd.grad(fz.sum(), depth2, retain_graph=True)
    (dlin_dimg,) = torch.autograd.grad(lin.sum(), img2, retain_graph=True)
    render = _RenderStageF64.apply(lin, fz, vol.psf, tables, ks, seen)
    loss_of(torch.clip(net.gamma(render), 0.0, 1.0)).backward()
    gl, gr = seen["G"][:, :C], seen["G"][:, C:]
    bar_fz = (16 * C * ks * ks + 8) * EPS * dfz_abs(lin.detach(), vol.psf, tables, gl, gr, ks)
    bar_img = (16 * ks * ks * fold_counts(H, W, ks).to(DEV) + 8) * EPS * dimg_abs(lin.detach(), vol.psf, tables, gl, gr, ks)
    for name, got, want, allowed in (
            ("depth", depth.grad, depth2.grad, bar_fz.unsqueeze(1) * dfz_ddepth.abs().double()),
            ("image", img.grad, img2.grad, bar_img * dlin_dimg.abs().double())):
        allowed = allowed + 4 * EPS * want.abs().double()
        diff = (got - want).abs().double()
        print(f"d loss / d {name}: largest |value| {float(want.abs().max()):.6e}, worst |fused - float64 stage| / allowed = "
              f"{float((diff / allowed.clamp_min(1e-300)).max()):.4f}")
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        assert bool((diff <= allowed).all())

    # demonstration: depth from the pair by analysis-by-synthesis, a few steps
    est = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([est], lr=40.0)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        step_loss = loss_of(net.render_volume(img0, est, vol, scene_grad=True))
        losses.append(float(step_loss.detach()))
        step_loss.backward()
        opt.step()
    with torch.no_grad():
        after = float(loss_of(net.render_volume(img0, est, vol)))
    err = lambda d: float((d.detach() - true_depth).abs().mean())
    print(f"Adam on the depth (lr 40 mm): loss {losses[0]:.6e} -> {after:.6e} over {len(losses)} steps "
          f"({', '.join(f'{l:.4e}' for l in losses)}); mean |depth - true| {err(start):.1f} -> {err(est):.1f} mm")
    assert after < losses[0]
