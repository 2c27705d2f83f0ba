"""The render from a PSF volume without a GPU: the float64 restatement (tests/render_volume_f64.py) against the
reference's own local_dp_psf_render run in float64 on the interpolated kernels, its interpolation against
torch.nn.functional.grid_sample and numpy.interp, axis_segments, the sampled evaluators against the full restatement,
and the C ABI of the two entries."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from render_volume_f64 import (interpolate_kernels, node_pixel_counts, render_volume_abs, render_volume_f64,
                               sampled_dvol, sampled_out, volume_grad_abs, volume_grad_f64)

from sdirt_amd.render_psf import PSFVolume, axis_segments, volume_segment_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, H, W, ks | Dz, Gy, Gx)
CASES = [(1, 3, 12, 17, 11, 3, 2, 3), (2, 1, 9, 7, 5, 3, 4, 4), (1, 4, 6, 11, 11, 2, 3, 2), (1, 3, 5, 9, 21, 2, 2, 2),
         (1, 3, 4, 5, 3, 3, 9, 11), (1, 3, 8, 9, 7, 1, 3, 3), (1, 3, 8, 9, 7, 3, 1, 1), (1, 1, 1, 1, 3, 2, 2, 2)]


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


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")
@pytest.mark.parametrize("case", CASES)
def test_restatement_and_its_gradient_are_the_references_in_float64(case):
    """The restatement's per-pixel kernels through the reference's local_dp_psf_render, and that graph's gradient in V
    (back through the interpolation): float64 sums of the same terms, 1e-12 of the largest value."""
    sys.path.insert(0, ROOT)
    from oracle._refimport import import_reference
    import_reference()
    from deeplens.render_psf import local_dp_psf_render
    b, c, h, w, ks = case[:5]
    img, vol, gl, gr, tables = operands(case)
    v = vol.clone().requires_grad_(True)
    ref = local_dp_psf_render(img, interpolate_kernels(v, tables), kernel_size=ks)
    left, right = render_volume_f64(img, vol, tables, ks)
    for got, want in ((left, ref[:, :c]), (right, ref[:, c:])):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    (torch.cat([gl, gr], 1) * ref).sum().backward()
    got = volume_grad_f64(img, vol.shape, tables, gl, gr, ks)
    assert got.shape == v.grad.shape
    assert float((got - v.grad).abs().max()) <= 1e-12 * float(v.grad.abs().max())


def test_interpolation_is_grid_sample_on_uniform_nodes():
    """Uniformly spaced nodes (y decreasing), coordinates inside and outside the node range and exactly on every node,
    all on a binary lattice so that the fp32 fractions of axis_segments are exact: the interpolated kernels of an
    h x w image are what grid_sample gives (5-D input, 'bilinear' = trilinear there, align_corners, border padding) in
    float64."""
    dz, gy, gx, ks, h, w = 3, 4, 5, 3, 23, 29
    gen = torch.Generator().manual_seed(1)
    vol = torch.randn((dz, gy, gx, 2, ks, ks), generator=gen, dtype=torch.float64)
    xn, yn, zn = torch.arange(gx) * 0.5 - 1.0, 0.75 - torch.arange(gy) * 0.5, torch.arange(dz) * 0.25
    pick = lambda lo, hi, *n: torch.randint(int(lo * 64) - 40, int(hi * 64) + 40, n, generator=gen) / 64.0
    tx, ty, tz = pick(-1.0, 1.0, w), pick(-0.75, 0.75, h), pick(0.0, 0.5, 1, h, w)
    tx[:gx], ty[:gy], tz[0, 0, :dz] = xn, yn, zn
    tables = (*axis_segments(xn, tx), *axis_segments(yn, ty), *axis_segments(zn, tz))
    got = interpolate_kernels(vol, tables)[0]                                        # [h,w,2,ks,ks]
    unit = lambda t, nodes: 2 * (t.double() - nodes[0]) / (nodes[-1] - nodes[0]) - 1
    grid = torch.stack((unit(tx, xn).reshape(1, w).expand(h, w), unit(ty, yn).reshape(h, 1).expand(h, w),
                        unit(tz[0], zn)), -1).reshape(1, 1, h, w, 3)
    field = vol.permute(3, 4, 5, 0, 1, 2).reshape(1, 2 * ks * ks, dz, gy, gx)
    want = torch.nn.functional.grid_sample(field, grid, mode="bilinear", padding_mode="border", align_corners=True)
    want = want.reshape(2, ks, ks, h, w).permute(3, 4, 0, 1, 2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(tx.min()) < -1.0 < 1.0 < float(tx.max()) and float(tz.min()) < 0.0 < 0.5 < float(tz.max())


def test_interpolation_is_numpy_interp_on_non_uniform_depth_nodes():
    """One (x, y) node, non-uniform z nodes, depths at exact quarters of every segment and outside both ends: every tap
    of the interpolated kernel is numpy.interp of that tap's node values."""
    ks = 3
    zn = torch.tensor([0.0, 0.125, 0.5, 1.0])
    gen = torch.Generator().manual_seed(2)
    vol = torch.randn((4, 1, 1, 2, ks, ks), generator=gen, dtype=torch.float64)
    z = torch.cat([zn[k] + (zn[k + 1] - zn[k]) * torch.arange(5) / 4 for k in range(3)] + [torch.tensor([-0.5, 1.75])])
    w = len(z)
    tables = volume_segment_tables(torch.tensor([0.0]), torch.tensor([0.0]), zn, z.reshape(1, 1, w), 1, w)
    k = interpolate_kernels(vol, tables)[0, 0]                                       # [w,2,ks,ks]
    for s in range(2):
        for i in range(ks):
            for j in range(ks):
                want = np.interp(z.double().numpy(), zn.double().numpy(), vol[:, 0, 0, s, i, j].numpy())
                assert np.abs(k[:, s, i, j].numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_axis_segments():
    dec = torch.tensor([0.75, 0.25, -0.5, -1.0])
    i, f = axis_segments(dec, dec)                                                   # exactly on every node
    assert i.tolist() == [0, 1, 2, 2] and f.tolist() == [0.0, 0.0, 0.0, 1.0]
    assert i.dtype == torch.int32 and f.dtype == torch.float32
    i, f = axis_segments(dec, torch.tensor([2.0, 0.5, 0.0, -0.75, -3.0]))            # outside both ends, inside
    assert i.tolist() == [0, 0, 1, 2, 2]
    assert torch.equal(f, torch.tensor([0.0, 0.5, np.float32(0.25) / np.float32(0.75), 0.5, 1.0]))
    inc = torch.tensor([0.0, 0.1, 1.0])
    i, f = axis_segments(inc, torch.tensor([[-1.0, 0.0, 0.05], [0.1, 1.0, 7.0]]))
    assert i.tolist() == [[0, 0, 0], [1, 1, 1]] and i.shape == (2, 3)
    assert torch.equal(f, torch.tensor([[0.0, 0.0, np.float32(0.05) / np.float32(0.1)], [0.0, 1.0, 1.0]]))
    i, f = axis_segments(torch.tensor([0.3]), torch.tensor([-2.0, 0.3, 5.0]))        # an axis of one node
    assert i.tolist() == [0, 0, 0] and f.tolist() == [0.0, 0.0, 0.0]
    assert not torch.signbit(axis_segments(dec, dec)[1]).any()
    with pytest.raises(ValueError):
        axis_segments(torch.tensor([0.0, 1.0, 0.5]), torch.tensor([0.2]))
    # every (i, f) stays inside the axis: i + 1 is a node
    i, f = axis_segments(dec, torch.linspace(-2, 2, 101))
    assert int(i.min()) == 0 and int(i.max()) == 2 and float(f.min()) >= 0 and float(f.max()) <= 1


@pytest.mark.parametrize("case", CASES)
def test_sampled_evaluators_are_the_full_restatement(case):
    """sampled_out / sampled_dvol at EVERY element: values, magnitudes and pixel counts."""
    b, c, h, w, ks, dz, gy, gx = case
    img, vol, gl, gr, tables = operands(case, seed=1)
    idx = torch.cartesian_prod(*[torch.arange(n) for n in (b, c, h, w)]).reshape(-1, 4)
    for absolute, full in ((False, render_volume_f64), (True, render_volume_abs)):
        left, right = full(img, vol, tables, ks)
        got = sampled_out(img, vol, tables, ks, idx, absolute)
        for s, want in enumerate((left, right)):
            assert float((got[:, s].reshape(want.shape) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    idx = torch.cartesian_prod(*[torch.arange(n) for n in (dz, gy, gx, 2, ks, ks)])
    counts = node_pixel_counts(tables, (dz, gy, gx))
    for absolute, full in ((False, volume_grad_f64), (True, volume_grad_abs)):
        want = full(img, vol.shape, tables, gl, gr, ks)
        got, n = sampled_dvol(img, gl, gr, tables, (dz, gy, gx), ks, idx, absolute)
        assert float((got.reshape(want.shape) - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert torch.equal(n.reshape(dz, gy, gx, -1), counts[..., None].expand(dz, gy, gx, 2 * ks * ks))
    # every pixel has weight at 1 ... 8 nodes; with more nodes than pixels some nodes have none
    assert b * h * w <= int(counts.sum()) <= 8 * b * h * w
    if dz * gy * gx > 8 * b * h * w:
        assert int((counts == 0).sum()) > 0


def test_psf_volume_points_are_in_volume_order():
    v = PSFVolume(None, torch.tensor([-0.5, 0.5]), torch.tensor([0.75, 0.0, -0.75]), torch.tensor([0.0, 0.5, 1.0, 0.25][:2]),
                  -200.0, -20000.0)
    p = v.points().reshape(2, 3, 2, 3)
    assert torch.equal(p[..., 0], torch.tensor([-0.5, 0.5]).expand(2, 3, 2))
    assert torch.equal(p[..., 1], torch.tensor([0.75, 0.0, -0.75]).reshape(1, 3, 1).expand(2, 3, 2))
    assert torch.equal(p[..., 2], torch.tensor([-200.0, -10100.0]).reshape(2, 1, 1).expand(2, 3, 2))


def test_volume_entries_are_declared_exported_and_refuse_bad_arguments():
    from sdirt_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    h = _lib.lib()
    P, I = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["sdirt_render_psf_volume"] == (ctypes.c_int, [P] * 8 + [I] * 8 + [P, P, P])
    assert _lib.SIGNATURES["sdirt_render_psf_volume_grad"] == (ctypes.c_int, [P] * 9 + [I] * 8 + [P, P])
    for name, pointers in (("sdirt_render_psf_volume", 8), ("sdirt_render_psf_volume_grad", 9)):
        assert hasattr(h, name)
        decl = header[header.index("int " + name + "("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        args = [a.strip() for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
        assert len(args) == pointers + 8 + (3 if pointers == 8 else 2), args
        assert all("*" in a for a in args[:pointers]) and all(a.startswith("int32_t ") for a in args[pointers:pointers + 8])
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert re.search(r"render_psf\.py:\d+", comment), name
    assert h.sdirt_abi_version() == 4
    # argument errors are statuses, returned before anything is launched: the pointers are never followed
    ptr = [ctypes.c_void_p(4096)] * 8
    shape = dict(B=1, C=3, H=8, W=8, ks=5, Dz=2, Gy=2, Gx=2)

    def forward(ptrs=ptr, out=(ptr[0], ptr[0]), **kw):
        s = {**shape, **kw}
        return h.sdirt_render_psf_volume(*ptrs, *s.values(), *out, None)

    def backward(ptrs=ptr + ptr[:1], out=ptr[0], **kw):
        s = {**shape, **kw}
        return h.sdirt_render_psf_volume_grad(*ptrs, *s.values(), out, None)

    for call in (forward, backward):
        assert call(ks=4) == -1 and b"odd" in h.sdirt_last_error()               # SDIRT_ERR_INVALID_ARGUMENT
        assert call(ks=0) == -1 and call(ks=-3) == -1
        assert call(ks=65) == -2 and b"63" in h.sdirt_last_error()               # SDIRT_ERR_UNSUPPORTED
        assert call(C=2) == -2 and call(C=0) == -2
        assert call(H=0) == -1 and call(W=0) == -1 and call(B=-1) == -1
        assert call(Dz=0) == -1 and call(Gy=0) == -1 and call(Gx=0) == -1
        assert call(out=None if call is backward else (None, ptr[0])) == -1
        for k in range(8 if call is forward else 9):
            ptrs = list(ptr + ptr[:1])[:8 if call is forward else 9]
            ptrs[k] = None
            assert call(ptrs=ptrs) == -1, k
    assert forward(out=(ptr[0], None)) == -1
    assert forward(B=0) == 0                                                     # an empty batch renders nothing


def test_calls_take_the_plain_path_unless_the_volume_requires_a_gradient(monkeypatch):
    """local_dp_psf_render_volume goes through the autograd Function only in grad mode with a volume that requires a
    gradient; an image or a depth that requires one is refused by name."""
    import importlib
    rp = importlib.import_module("sdirt_amd.render_psf")
    seen = []
    monkeypatch.setattr(rp, "_render_volume", lambda i, v, t, ks: seen.append("plain") or (i, i))
    monkeypatch.setattr(rp._RenderPsfVolume, "apply", lambda v, i, *a: seen.append("grad") or torch.cat([i, i], 1))
    img, vol, z = torch.zeros(1, 3, 4, 4), torch.zeros(2, 2, 2, 2, 3, 3), torch.zeros(1, 4, 4)
    nodes = (torch.tensor([-1.0, 1.0]), torch.tensor([1.0, -1.0]), torch.tensor([0.0, 1.0]))
    call = lambda i, v, zz=z: rp.local_dp_psf_render_volume(i, v, *nodes, zz, 3)
    assert call(img, vol).shape == (1, 6, 4, 4)
    with torch.no_grad():
        call(img.clone().requires_grad_(True), vol.clone().requires_grad_(True), z.clone().requires_grad_(True))
    call(img, vol.clone().requires_grad_(True))
    assert seen == ["plain", "plain", "grad"]
    with pytest.raises(ValueError, match="image"):
        call(img.clone().requires_grad_(True), vol)
    with pytest.raises(ValueError, match="depth"):
        call(img, vol, z.clone().requires_grad_(True))
