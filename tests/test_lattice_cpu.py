"""The lattice inputs and float64 restatements of tests/lattice_f64.py checked on the reference alone (no GPU): the
conditions under which tests/test_gpu_lattice.py may ask the kernels for bit equality, and the restatements against
independent forms of the same arithmetic."""
import copy

import numpy as np
import pytest
import torch

import lattice_f64 as L
from conftest import load_golden

# rows per network on the CPU: the largest row count of its GPU cases (the persistent-loop case, whose row count
# follows the device's CU count and which asserts the same conditions on its own points, stands in with 1000)
CPU_ROWS = {L.NET_PRODUCTION: 300, L.NET_3_LAYERS: 129, L.NET_16_LAYERS: 200, L.NET_PERSISTENT: 1000}


@pytest.mark.parametrize("cfg", L.MLP_NETS, ids=lambda c: "h4_%d-hidden_%d-out_%d-nnz_%d" % c[1:])
def test_lattice_mlp_sums_are_exact_and_alive(cfg):
    net, weights, biases = L.lattice_mlp(*cfg)
    assert net.fused_supported() and len(weights) == cfg[2] + 3
    for l, (w, b) in enumerate(zip(weights, biases)):
        assert torch.equal(w, w.round()) and float(w.abs().max()) <= (2 if l == 0 else 1)
        assert torch.equal(b / L.U, (b / L.U).round()) and -4 <= float(b.min() / L.U) and float(b.max() / L.U) <= 8
        if l > 0:
            nnz = (w != 0).sum(1)
            assert int(nnz.min()) >= 1 and int(nnz.max()) <= cfg[4]
    x = L.mlp_points(cfg, CPU_ROWS.get(cfg, 129))
    assert torch.equal(x, x.half().float()) and torch.equal(x / L.U, (x / L.U).round())
    out, report = L.mlp_f64(weights, biases, x)
    print(cfg, report)
    L.assert_mlp_exact(report)
    for l, r in enumerate(report):
        assert r["nonzero"] >= 0.3, (l, r)
    assert torch.equal(out / L.U, (out / L.U).round())                  # still on the lattice
    if cfg in (L.NET_PRODUCTION, L.NET_16_LAYERS):
        # deep enough for fp16 to lose multiples of u: round-to-nearest-even decides a good share of the bits
        assert report[-1]["rounded"] > 0.2 and report[-1]["amax"] > 1000, report[-1]
    # the module's own layers in float64, the fp16 rounding applied by hand
    h = x.double()
    for m in copy.deepcopy(net).double().net:
        h = m(h)
        if isinstance(m, torch.nn.ReLU):
            h = torch.from_numpy(h.detach().numpy().astype(np.float16).astype(np.float64))
    assert torch.equal(h, out)


def test_lattice_points_cover_the_input_range():
    x = L.lattice_points(3, 500)
    assert x.shape == (500, 3) and x.dtype == torch.float32
    assert float(x[:, :2].abs().max()) <= 1 and float(x[:, 2].min()) >= 0 and float(x[:, 2].max()) <= 1
    assert len(torch.unique(x[:, 0])) > 50 and len(torch.unique(x[:, 2])) > 25


@pytest.mark.parametrize("shape", [(1, 3, 5, 9, 21), (2, 1, 4, 6, 7), (1, 4, 2, 3, 65)])
def test_lattice_render_products_and_sums_are_exact(shape):
    """render_f64 on lattice inputs == the same sum with every product rounded to fp16: the products are exact in
    fp16; and every sum of magnitudes is below 2^24 units of 2^-11: any fp32 summation order is exact."""
    B, C, H, W, ks = shape
    img, psf = L.lattice_image(sum(shape), B, C, H, W), L.lattice_psf(sum(shape) + 1, B, H, W, ks)
    assert float(img.max()) == 31 / 32 and float(psf.max()) == 63 / 64 and float(img.min()) == 0 == float(psf.min())
    assert torch.equal(img, img.half().float()) and torch.equal(psf, psf.half().float())
    left, right = L.render_f64(img.double(), psf.double(), ks)
    hl, hr, al, ar = L.render_f16_products_f64(img, psf, ks)
    assert torch.equal(left, hl) and torch.equal(right, hr)
    assert torch.equal(left, al) and torch.equal(right, ar)             # no negative terms
    assert float(torch.maximum(al, ar).max()) * 2 ** 11 < L.EXACT
    assert 65 * 65 * 31 * 63 < L.EXACT                                  # whatever the draw, up to ks 65
    assert torch.equal(left, left.float().double())                     # the result is an fp32 number
    assert float(left.max()) < 65504                                    # ... and within fp16's range


def test_fp16_restatement_against_the_reference_renderer():
    """render_f16_products_f64 on fixture f7 (render_psf.py:120-155 on random normalised kernels, ks 5) rounded to
    fp16: within one fp16 ulp of the reference's fast_l / fast_r (whose unfold-and-sum adds in another order and
    rounds its partial sums), mostly bit-equal."""
    g = load_golden("f7_render")
    img, psf, ks = torch.from_numpy(g["img"]), torch.from_numpy(g["psf"]), int(g["ks"])
    left, right, _, _ = L.render_f16_products_f64(img, psf, ks)
    for got, key in ((left, "fast_l"), (right, "fast_r")):
        ref = torch.from_numpy(g[key]).double()
        err = (L.round_f16(got) - ref).abs()
        assert bool((err <= 2 * L.half_ulp(ref)).all()), float(err.max())
        assert float((L.round_f16(got) == ref).double().mean()) >= 0.9


def test_half_ulp_is_half_the_fp16_spacing():
    x = np.array([1.0, 0.999, 0.3, 0.25, 2047.9, 1e-3, 2.0 ** -14, 65000.0])
    want = np.spacing(x.astype(np.float16)).astype(np.float64) / 2
    # np.spacing of a rounded-up value belongs to the upper binade: compare on fp16 values
    got = L.half_ulp(torch.from_numpy(x.astype(np.float16).astype(np.float64)))
    assert np.array_equal(got.numpy(), want)
    assert L.half_ulp(torch.tensor([0.0, 1e-7, -0.75])).tolist() == [2.0 ** -25, 2.0 ** -25, 2.0 ** -12]


@pytest.mark.parametrize("ks", sorted({s[-1] for s in L.PSFNET_SHAPES}))
def test_lattice_raw_keeps_weights_and_products_normal(ks):
    raw_l, raw_r = L.lattice_raw(ks, 2, 3, 5, ks)
    assert raw_l.dtype == torch.float16 and raw_l.shape == (2, 3, 5, ks, ks)
    m = torch.stack((raw_l, raw_r)).double() * 1024
    assert torch.equal(m, m.round()) and float(m[m > 0].min()) >= 128 and float(m.max()) <= L.raw_m_hi(ks) < 2048
    assert 0.15 < float((m == 0).double().mean()) < 0.35
    assert ks * ks * L.raw_m_hi(ks) < L.EXACT                           # the kernel's fp32 sum of a kernel is exact
    w = L.psfnet_weights(raw_l, raw_r, ks).double()
    assert float(w[w > 0].min()) >= 2.0 ** -12                          # times an image value >= 1/4: >= 2^-14
    img = L.lattice_image(ks, 2, 3, 3, 5, floor=8)
    assert set(torch.unique(img * 32).tolist()) <= {0.0, *map(float, range(8, 32))}
    assert abs(float(w.sum((-1, -2)).mean()) - 1) < 2e-3


def test_psfnet_render_f64_against_a_pixel_by_pixel_loop():
    """psfnet_render_f64 on a tiny case == PSFNet.pred's stack / fliplr / normalise and the _fast renderer written
    out pixel by pixel and tap by tap in numpy scalars; a dead kernel renders exactly 0 on its side."""
    B, C, H, W, ks = 1, 2, 3, 4, 3
    pad = 1
    raw_l, raw_r = L.lattice_raw(11, B, H, W, ks)
    raw_l[0, 1, 2] = 0
    raw_r[0, 0, 3] = 0
    img = L.lattice_image(12, B, C, H, W, floor=8)
    left, right, al, ar = L.psfnet_render_f64(img, raw_l, raw_r, ks)
    f16, f32 = np.float16, np.float32
    want = np.zeros((2, C, H, W))
    for y in range(H):
        for x in range(W):
            for s, raw in enumerate((raw_l[0, y, x].numpy(), raw_r[0, y, x].numpy()[:, ::-1])):
                tot = f16(raw.astype(np.float64).sum())
                inv = f32(1) / (f32(tot) + f32(1e-9))
                for i in range(ks):
                    for j in range(ks):
                        wt = f16(f32(raw[i, j]) * inv)
                        yy, xx = min(max(y + pad - i, 0), H - 1), min(max(x + pad - j, 0), W - 1)
                        for c in range(C):
                            want[s, c, y, x] += float(f16(f16(img[0, c, yy, xx].item()) * wt))
    assert np.array_equal(left[0].numpy(), want[0]) and np.array_equal(right[0].numpy(), want[1])
    assert torch.equal(al, left) and torch.equal(ar, right)
    assert float(left[0, :, 1, 2].abs().max()) == 0 and float(right[0, :, 0, 3].abs().max()) == 0
    assert float(left.max()) < 1 and float(left.max()) > 0.3
