"""The scene gradients of the render from a PSF volume without a GPU: the float64 restatement
(tests/render_volume_scene_f64.py) against central differences, its depth gradient chained to z against
torch.nn.functional.grid_sample's autograd, the sampled evaluators against the full restatement, the z -> fz convention
of axis_segments at the nodes, the C ABI of sdirt_render_psf_volume_grad_scene and the routing of scene_grad."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from render_f64 import render_f64
from render_volume_f64 import interpolate_kernels
from render_volume_scene_f64 import (dfz_abs, dimg_abs, fold_counts, sampled_dfz, sampled_dimg, scene_grads_f64)

from sdirt_amd.render_psf import axis_segments, volume_segment_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, H, W, ks | Dz, Gy, Gx): an image smaller than pad, one row, one column, a batch, one depth node, one pixel
CASES = [(1, 3, 12, 17, 11, 3, 2, 3), (2, 1, 9, 7, 5, 3, 4, 4), (1, 4, 6, 11, 11, 2, 3, 2), (1, 3, 5, 9, 21, 2, 2, 2),
         (1, 3, 1, 7, 5, 2, 2, 2), (1, 3, 7, 1, 5, 3, 2, 2), (1, 3, 8, 9, 7, 1, 3, 3), (1, 1, 1, 1, 3, 2, 2, 2)]


def nodes_for(dz, gy, gx, gen):
    """Cell-centred x, decreasing y, non-uniform increasing z."""
    x = torch.linspace(-1 + 1 / (2 * gx), 1 - 1 / (2 * gx), gx) if gx > 1 else torch.tensor([0.1])
    y = torch.linspace(1 - 1 / (2 * gy), -1 + 1 / (2 * gy), gy) if gy > 1 else torch.tensor([-0.2])
    z = torch.cumsum(torch.rand(dz, generator=gen) + 0.05, 0)
    return x, y, (z - z[0]) / (z[-1] - z[0]) if dz > 1 else torch.tensor([0.4])


def operands(case, seed=0):
    b, c, h, w, ks, dz, gy, gx = case
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    x, y, z = nodes_for(dz, gy, gx, gen)
    depth = torch.rand((b, h, w), generator=gen) * 1.4 - 0.2                     # partly outside [0, 1] at both ends
    depth.view(-1)[:min(dz, depth.numel())] = z[:depth.numel()]                  # and some exactly on nodes
    tables = volume_segment_tables(x, y, z, depth, h, w)
    return rnd(b, c, h, w), rnd(dz, gy, gx, 2, ks, ks), rnd(b, c, h, w), rnd(b, c, h, w), tables


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4], CASES[6]])
def test_restatement_against_central_differences(case):
    """The loss is linear in the image and in fz, so a central difference has no truncation error: 1e-9 of the largest
    gradient (or of the loss's magnitude sum, where the gradient is 0), at a fixed sample of elements of both."""
    b, c, h, w, ks, dz, gy, gx = case
    img, vol, gl, gr, tables = operands(case)
    fz = tables[5].double()

    def loss(image, frac):
        left, right = render_f64(image, interpolate_kernels(vol, (*tables[:5], frac)), ks)
        return float((gl * left).sum() + (gr * right).sum())

    dimg, dfz = scene_grads_f64(img, vol, tables, gl, gr, ks)
    assert dimg.shape == img.shape and dfz.shape == fz.shape
    # the difference of two float64 losses carries their rounding, 2^-52 sum|terms| / step: far below 1e-9 sum|terms|
    left, right = render_f64(img.abs(), interpolate_kernels(vol.abs(), tables), ks)
    noise = float((gl.abs() * left).sum() + (gr.abs() * right).sum())
    gen = torch.Generator().manual_seed(7)
    step = 2.0 ** -10
    for flat in torch.randint(0, img.numel(), (12,), generator=gen).tolist() + [0, img.numel() - 1]:
        e = torch.zeros_like(img).view(-1)
        e[flat] = step
        e = e.view_as(img)
        fd = (loss(img + e, fz) - loss(img - e, fz)) / (2 * step)
        assert abs(fd - float(dimg.view(-1)[flat])) <= 1e-9 * max(float(dimg.abs().max()), noise)
    for flat in torch.randint(0, fz.numel(), (12,), generator=gen).tolist() + [0, fz.numel() - 1]:
        e = torch.zeros_like(fz).view(-1)
        e[flat] = step
        e = e.view_as(fz)
        fd = (loss(img, fz + e) - loss(img, fz - e)) / (2 * step)
        assert abs(fd - float(dfz.view(-1)[flat])) <= 1e-9 * max(float(dfz.abs().max()), noise)
    if dz == 1:
        assert not dfz.any()
    else:
        assert float(dfz.abs().max()) > 0


def test_depth_gradient_chained_to_z_is_grid_sample_autograd():
    """Uniform nodes on a binary lattice (y decreasing), depths inside and outside the node range and on the interior
    node: dfz of the restatement times the slope torch's autograd gives axis_segments is what autograd gives grid_sample
    (5-D, align_corners, border padding) in the grid's z coordinate, chained to z, to 1e-10.  (The two end nodes are
    left out: exactly there grid_sample's border clipping gives 0 at the first and differentiates towards a neighbour
    outside the volume at the last, where torch.clamp -- the convention here, pinned in the next test -- passes the
    segment's slope.)"""
    dz, gy, gx, ks, h, w, c = 3, 4, 5, 3, 11, 13, 2
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    vol, img, gl, gr = rnd(dz, gy, gx, 2, ks, ks), rnd(1, c, h, w), rnd(1, c, h, w), rnd(1, c, h, w)
    xn, yn, zn = torch.arange(gx) * 0.5 - 1.0, 0.75 - torch.arange(gy) * 0.5, torch.arange(dz) * 0.25
    pick = lambda lo, hi, *n: torch.randint(int(lo * 64) - 40, int(hi * 64) + 40, n, generator=gen) / 64.0
    tx, ty, tz = pick(-1.0, 1.0, w), pick(-0.75, 0.75, h), pick(0.0, 0.5, 1, h, w)
    tz[tz == zn[-1]] += 1 / 64.0
    tz[tz == zn[0]] -= 1 / 64.0
    tz[0, 0, :3] = zn[1]
    z32 = tz.clone().requires_grad_(True)
    iz, fz = axis_segments(zn, z32)
    assert fz.requires_grad and iz.dtype == torch.int32
    slope = torch.autograd.grad(fz.sum(), z32)[0]
    tables = (*axis_segments(xn, tx), *axis_segments(yn, ty), iz, fz.detach())
    got = scene_grads_f64(img, vol, tables, gl, gr, ks)[1] * slope.double()

    z64 = tz.double().requires_grad_(True)
    unit = lambda t, nodes: 2 * (t.double() - nodes[0]) / (nodes[-1] - nodes[0]) - 1
    grid = torch.stack((unit(tx, xn).reshape(1, w).expand(h, w), unit(ty, yn).reshape(h, 1).expand(h, w),
                        unit(z64[0], zn)), -1).reshape(1, 1, h, w, 3)
    field = vol.permute(3, 4, 5, 0, 1, 2).reshape(1, 2 * ks * ks, dz, gy, gx)
    k = torch.nn.functional.grid_sample(field, grid, mode="bilinear", padding_mode="border", align_corners=True)
    left, right = render_f64(img, k.reshape(2, ks, ks, h, w).permute(3, 4, 0, 1, 2).unsqueeze(0), ks)
    want = torch.autograd.grad((gl * left).sum() + (gr * right).sum(), z64)[0]
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())
    outside = (tz < 0) | (tz > 0.5)
    assert int(outside.sum()) > 0 and not got[outside].any() and got[~outside].all()


def test_axis_segments_is_differentiable_with_torchs_convention_at_the_kinks():
    """The slope of the segment the table names, also exactly on a node (end nodes included); exactly 0 outside."""
    nodes = torch.tensor([0.0, 0.3, 1.0])
    z = torch.tensor([0.0, 0.1, 0.3, 0.5, 1.0, -0.2, 1.5], requires_grad=True)
    i, f = axis_segments(nodes, z)
    assert i.dtype == torch.int32 and i.tolist() == [0, 0, 1, 1, 1, 0, 1] and f.requires_grad
    (slope,) = torch.autograd.grad(f.sum(), z)
    first = np.float32(1) / (np.float32(0.3) - np.float32(0.0))
    second = np.float32(1) / (np.float32(1.0) - np.float32(0.3))
    assert slope.tolist() == [first, first, second, second, second, 0.0, 0.0]
    assert abs(first - 3.3333) < 1e-3 and abs(second - 1.4286) < 1e-4
    dec = torch.tensor([0.75, 0.25, -0.5])                                           # a decreasing axis: negative slopes
    z = torch.tensor([0.75, 0.5, 0.25, -0.5, 2.0, -3.0], requires_grad=True)
    (slope,) = torch.autograd.grad(axis_segments(dec, z)[1].sum(), z)
    assert slope.tolist() == [-2.0, -2.0, np.float32(1) / np.float32(-0.75), np.float32(1) / np.float32(-0.75), 0.0, 0.0]
    one = torch.tensor([0.1, 0.9], requires_grad=True)                               # an axis of one node: no graph
    assert not axis_segments(torch.tensor([0.4]), one)[1].requires_grad


@pytest.mark.parametrize("case", CASES)
def test_sampled_evaluators_are_the_full_restatement(case):
    """sampled_dimg / sampled_dfz at EVERY element, values and magnitudes; the fold counts against a count by hand."""
    b, c, h, w, ks, dz, gy, gx = case
    img, vol, gl, gr, tables = operands(case, seed=1)
    dimg, dfz = scene_grads_f64(img, vol, tables, gl, gr, ks)
    pairs = ((False, dimg, dfz), (True, dimg_abs(img, vol, tables, gl, gr, ks), dfz_abs(img, vol, tables, gl, gr, ks)))
    idx4 = torch.cartesian_prod(*[torch.arange(n) for n in (b, c, h, w)]).reshape(-1, 4)
    idx3 = torch.cartesian_prod(*[torch.arange(n) for n in (b, h, w)]).reshape(-1, 3)
    for absolute, want_img, want_fz in pairs:
        got = sampled_dimg(vol, gl, gr, tables, ks, idx4, absolute).reshape(want_img.shape)
        assert float((got - want_img).abs().max()) <= 1e-12 * float(want_img.abs().max())
        got = sampled_dfz(img, vol, gl, gr, tables, ks, idx3, absolute).reshape(want_fz.shape)
        assert float((got - want_fz).abs().max()) <= 1e-12 * float(want_fz.abs().max())
    assert bool((pairs[1][1] >= dimg.abs() * (1 - 1e-12)).all()) and bool((pairs[1][2] >= dfz.abs() * (1 - 1e-12)).all())
    if dz == 1:
        assert not dfz.any()
    pad = (ks - 1) // 2
    m = fold_counts(h, w, ks)
    by_hand = torch.zeros(h, w, dtype=torch.long)
    for vp in range(-pad, h + pad):
        for up in range(-pad, w + pad):
            by_hand[min(max(vp, 0), h - 1), min(max(up, 0), w - 1)] += 1
    assert torch.equal(m, by_hand)


def test_scene_entry_is_declared_exported_and_refuses_bad_arguments():
    from sdirt_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    h = _lib.lib()
    P, I = ctypes.c_void_p, ctypes.c_int32
    name = "sdirt_render_psf_volume_grad_scene"
    assert _lib.SIGNATURES[name] == (ctypes.c_int, [P] * 10 + [I] * 8 + [P, P, P])
    assert hasattr(h, name)
    decl = header[header.index("int " + name + "("):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    args = [a.strip() for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert len(args) == 10 + 8 + 3, args
    assert all("*" in a for a in args[:10] + args[18:]) and all(a.startswith("int32_t ") for a in args[10:18])
    comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
    assert re.search(r"render_psf\.py:157-188", comment)
    assert h.sdirt_abi_version() == 4 and "#define SDIRT_ABI_VERSION 4" in re.sub(r"[ \t]+", " ", header)
    # argument errors are statuses, returned before anything is launched: the pointers are never followed
    ptr = [ctypes.c_void_p(4096)] * 10
    shape = dict(B=1, C=3, H=8, W=8, ks=5, Dz=2, Gy=2, Gx=2)

    def call(ptrs=ptr, out=(ptr[0], ptr[0]), **kw):
        s = {**shape, **kw}
        return getattr(h, name)(*ptrs, *s.values(), *out, None)

    assert call(ks=4) == -1 and b"odd" in h.sdirt_last_error()                   # SDIRT_ERR_INVALID_ARGUMENT
    assert call(ks=0) == -1 and call(ks=-3) == -1
    assert call(ks=65) == -2 and b"63" in h.sdirt_last_error()                   # SDIRT_ERR_UNSUPPORTED
    assert call(C=2) == -2 and call(C=0) == -2
    assert call(H=0) == -1 and call(W=0) == -1 and call(B=-1) == -1
    assert call(Dz=0) == -1 and call(Gy=0) == -1 and call(Gx=0) == -1
    assert call(B=65536) == -2 and call(H=65536) == -2
    assert call(out=(None, None)) == -1                                          # neither gradient asked for
    for k in range(10):
        ptrs = list(ptr)
        ptrs[k] = None
        assert call(ptrs=ptrs) == -1, k
    # an empty batch is SDIRT_OK with either output left out, and nothing is launched
    assert call(B=0) == 0 and call(B=0, out=(None, ptr[0])) == 0 and call(B=0, out=(ptr[0], None)) == 0


class _FakeLib:
    """Records which gradient entries a backward calls and which outputs it asks of the scene entry."""

    def __init__(self):
        self.calls = []

    def sdirt_render_psf_volume_grad(self, *args):
        assert len(args) == 19 and args[17] is not None
        self.calls.append("volume")
        return 0

    def sdirt_render_psf_volume_grad_scene(self, *args):
        assert len(args) == 21
        self.calls.append(("scene", args[18] is not None, args[19] is not None))
        return 0


def test_scene_grad_routing_and_what_the_backward_calls(monkeypatch):
    """scene_grad=False is today's call, refusals included; scene_grad=True in grad mode with anything requiring a
    gradient goes through _RenderPsfVolumeScene, otherwise through the plain call; the backward calls only the entries
    ctx.needs_input_grad names, with NULL for the output that is not wanted."""
    import importlib
    rp = importlib.import_module("sdirt_amd.render_psf")
    seen, fake = [], _FakeLib()
    monkeypatch.setattr(rp, "_render_volume", lambda i, v, t, ks: seen.append("kernel") or (i * 1.0, i * 1.0))
    monkeypatch.setattr(rp, "stream_ptr", lambda device=None: None)
    monkeypatch.setattr(rp._lib, "lib", lambda: fake)
    scene_apply = rp._RenderPsfVolumeScene.apply
    monkeypatch.setattr(rp._RenderPsfVolumeScene, "apply", lambda *a: seen.append("scene") or scene_apply(*a))
    monkeypatch.setattr(rp._RenderPsfVolume, "apply", lambda v, i, *a: seen.append("volume") or torch.cat([i, i], 1))
    img, vol, z = torch.zeros(1, 3, 4, 4), torch.zeros(2, 2, 2, 2, 3, 3), torch.full((1, 4, 4), 0.25)
    nodes = (torch.tensor([-1.0, 1.0]), torch.tensor([1.0, -1.0]), torch.tensor([0.0, 1.0]))
    leaf = lambda t: t.clone().requires_grad_(True)

    def call(i, v, zz, **kw):
        del seen[:]
        return rp.local_dp_psf_render_volume(i, v, *nodes, zz, 3, **kw)

    # the default: refusals as before, the volume's Function as before
    with pytest.raises(ValueError, match="image"):
        call(leaf(img), vol, z)
    with pytest.raises(ValueError, match="depth"):
        call(img, vol, leaf(z), scene_grad=False)
    call(img, leaf(vol), z)
    assert seen == ["volume"]
    # opted in, but nothing to record
    assert call(img, vol, z, scene_grad=True).shape == (1, 6, 4, 4) and seen == ["kernel"]
    with torch.no_grad():
        call(leaf(img), leaf(vol), leaf(z), scene_grad=True)
    assert seen == ["kernel"]
    # opted in: every combination of leaves reaches the new Function, and its backward asks for exactly those
    for want_v, want_i, want_z in [(0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)]:
        i, v, zz = (leaf(t) if on else t for t, on in ((img, want_i), (vol, want_v), (z, want_z)))
        out = call(i.half() if want_i else i, v, zz, scene_grad=True)
        assert seen == ["scene", "kernel"] and out.grad_fn is not None
        assert out.dtype == (torch.float16 if want_i else torch.float32)
        del fake.calls[:]
        out.sum().backward()
        expected = (["volume"] if want_v else []) + ([("scene", bool(want_i), bool(want_z))] if want_i or want_z else [])
        assert fake.calls == expected, (want_v, want_i, want_z, fake.calls)
        assert (i.grad is not None) == bool(want_i) and (v.grad is not None) == bool(want_v)
        assert (zz.grad is not None) == bool(want_z)
        if want_i:
            assert i.grad.dtype == i.dtype and i.grad.shape == i.shape
        if want_z:
            assert zz.grad.shape == zz.shape
    # an axis of one depth node: z.grad is 0, not missing
    zz = leaf(z)
    nodes = (nodes[0], nodes[1], torch.tensor([0.4]))
    out = call(img, vol[:1], zz, scene_grad=True)
    fake_fz = []

    def zero_dfz(*a):                                    # what the kernel writes where both depth planes are one node
        fake_fz.append(a[19] is not None)
        ctypes.memset(a[19], 0, 4 * z.numel())
        return 0

    monkeypatch.setattr(fake, "sdirt_render_psf_volume_grad_scene", zero_dfz)
    out.sum().backward()
    assert fake_fz == [True] and zz.grad is not None and not zz.grad.any()
