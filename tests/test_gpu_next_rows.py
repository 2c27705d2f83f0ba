"""GPU tests of the rows either side of the hot path: the
image-space per-pixel PSF convolution (f1), the PSFNet data generators (f2) and
this package's own geometric optics (f3)."""
import os

import numpy as np
import pytest
import torch

from conftest import DATA, load_golden, load_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def test_local_psf_render_against_reference():
    """render_psf.py:76-188 on the f7 fixture (B=2, C=3, 8x12 image, ks 5)."""
    from sdirt_amd import local_dp_psf_render, local_psf_render, local_psf_render_fast
    g = load_golden("f7_render")
    img, psf, ks = t(g["img"]), t(g["psf"]), int(g["ks"])
    out = local_dp_psf_render(img, psf, kernel_size=ks)                 # fp32 path
    assert out.shape == g["dp_fp32"].shape
    assert np.abs(out.cpu().numpy() - g["dp_fp32"]).max() < 2e-6
    for fn, key in ((local_psf_render_fast, "fast"), (local_psf_render, "half")):
        rl, rr = fn(img, psf, kernel_size=ks)                           # fp16 arithmetic
        assert rl.dtype == torch.float32 and rl.shape == g[key + "_l"].shape
        # one fp16 ulp at values < 1 is 4.9e-4; the reference itself differs from the
        # fp32 result by 3e-4
        assert np.abs(rl.cpu().numpy() - g[key + "_l"]).max() <= 5e-4
        assert np.abs(rr.cpu().numpy() - g[key + "_r"]).max() <= 5e-4
        assert np.mean(rl.cpu().numpy() == g[key + "_l"]) > 0.9         # mostly bit-equal fp16 values
    # replicate padding + flipped kernel: a delta kernel at tap (0,0) shifts the image by (+pad,+pad)
    d = torch.zeros(1, 8, 12, 2, ks, ks, device=DEV)
    d[..., 0, 0] = 1.0
    rl, _ = local_psf_render_fast(img[:1], d, kernel_size=ks)
    pad = (ks - 1) // 2
    exp = torch.nn.functional.pad(img[:1], (pad, pad, pad, pad), mode="replicate")[..., 2 * pad:, 2 * pad:]
    assert torch.allclose(rl, exp.half().float(), atol=0)
    # the same check is exact in fp16 arithmetic on every dispatch path: ks 5 (8 pixels per LDS tile), 21 (C 3: the
    # wave-per-pixel kernel), 33 (4 per tile), 49 (2 per tile), 65 (direct kernel), 1 / 3 / 4 channels each; images
    # a little larger than pad so that the shifted image is not one replicated corner.  A one-hot at the first tap
    # shifts by (+pad,+pad), one at the last tap (ks-1,ks-1) by (-pad,-pad): the last lanes of the tap tiling and
    # the flip in the other direction.  Both sides get both taps (`kr` is the second half of a pixel's run).
    gen = torch.Generator(device=DEV).manual_seed(7)
    for ks in (5, 21, 33, 49, 65):
        pad = (ks - 1) // 2
        H, W = pad + 5, pad + 9
        for C in (1, 3, 4):
            x = torch.rand(1, C, H, W, device=DEV, generator=gen)
            padded = torch.nn.functional.pad(x, (pad, pad, pad, pad), mode="replicate")
            first, last = padded[..., 2 * pad:, 2 * pad:].half().float(), padded[..., :H, :W].half().float()
            for tl, tr in ((0, ks - 1), (ks - 1, 0)):
                d = torch.zeros(1, H, W, 2, ks, ks, device=DEV)
                d[..., 0, tl, tl] = 1.0
                d[..., 1, tr, tr] = 1.0
                rl, rr = local_psf_render_fast(x, d, kernel_size=ks)
                assert torch.allclose(rl, first if tl == 0 else last, atol=0), (ks, C, tl)
                assert torch.allclose(rr, first if tr == 0 else last, atol=0), (ks, C, tr)


def test_local_psf_render_high_res_against_reference_tiles():
    """render_psf.py:191-208 (fixture F18: the reference's local_psf_render applied tile by tile, which
    is what the reference's loop computes; its own function raises on the (left, right) tuple)."""
    from sdirt_amd import local_psf_render, local_psf_render_high_res
    g = load_golden("f18_render_high_res")
    img, psf, ks = t(g["img"]), t(g["psf"]), int(g["ks"])
    rl, rr = local_psf_render_high_res(img, psf, patch_size=[int(v) for v in g["patch"]], kernel_size=ks)
    assert rl.shape == img.shape
    assert np.abs(rl.cpu().numpy() - g["left"]).max() <= 5e-4 and np.abs(rr.cpu().numpy() - g["right"]).max() <= 5e-4
    assert np.mean(rl.cpu().numpy() == g["left"]) > 0.9
    # one tile covering the image is the plain renderer; interior tiles differ from it (own padding)
    whole_l, _ = local_psf_render(img, psf, kernel_size=ks)
    one_l, _ = local_psf_render_high_res(img, psf, patch_size=[64, 64], kernel_size=ks)
    assert torch.equal(whole_l, one_l)
    assert not torch.equal(whole_l, rl)


@pytest.mark.parametrize("shape", [(2, 3, 9, 13, 21), (1, 3, 5, 8, 21), (1, 3, 33, 70, 21), (1, 3, 4, 97, 21),
                                   (1, 1, 7, 10, 21), (1, 3, 6, 11, 7), (1, 4, 5, 9, 33), (1, 3, 5, 9, 49),
                                   (1, 1, 4, 7, 65)])
def test_render_kernels_equal_a_plain_torch_convolution(shape):
    """The dispatch paths of sdirt_local_psf_render in fp32: the software-pipelined wave-per-pixel kernel
    (ks 21 RGB), the row-mapped LDS-tiled kernel with 8 (ks 21 C 1, ks 7), 4 (ks 33) and 2 (ks 49) pixels
    per tile, the direct kernel (ks 65) -- on ragged shapes: rows shorter than a pixel group, widths that
    are not a multiple of 8, odd run alignments, the tensor's last partial 16-byte vector -- against the
    definition: replicate padding, flipped per-pixel kernels, fp32.  Not reached: the direct kernel as
    the fallback of ks <= 64 for images beyond 32-bit offsets (C*H*W >= 2^30 elements or B*H >= 65536),
    which no small input selects."""
    from sdirt_amd import local_dp_psf_render
    B, C, H, W, ks = shape
    g = torch.Generator(device=DEV).manual_seed(sum(shape))
    img = torch.rand(B, C, H, W, device=DEV, generator=g)
    psf = torch.rand(B, H, W, 2, ks, ks, device=DEV, generator=g)
    out = local_dp_psf_render(img, psf, kernel_size=ks)                       # [B, 2C, H, W]
    pad = (ks - 1) // 2
    patches = torch.nn.functional.unfold(torch.nn.functional.pad(img.double(), (pad,) * 4, mode="replicate"),
                                         (ks, ks)).view(B, C, ks * ks, H * W)
    k = torch.flip(psf.double(), [-2, -1]).view(B, H * W, 2, ks * ks).permute(0, 2, 3, 1)   # [B,2,ks*ks,HW]
    ref = torch.cat([(patches * k[:, s:s + 1]).sum(2).view(B, C, H, W) for s in (0, 1)], dim=1)
    assert torch.allclose(out.double(), ref, rtol=0, atol=2e-5 * float(ref.max()))


def test_render_production_size_runs_and_conserves_energy():
    """512x768, ks 21 (config 5 of BASELINE.json): normalised kernels keep a flat image flat."""
    from sdirt_amd import local_psf_render_fast
    H, W, ks = 512, 768, 21
    g = torch.Generator(device=DEV).manual_seed(0)
    psf = torch.rand(1, H, W, 2, ks, ks, device=DEV, generator=g)
    psf = psf / psf.sum((-1, -2), keepdim=True)
    img = torch.full((1, 3, H, W), 0.5, device=DEV)
    rl, rr = local_psf_render_fast(img, psf, kernel_size=ks)
    assert rl.shape == (1, 3, H, W)
    assert (rl - 0.5).abs().max() < 2e-3 and (rr - 0.5).abs().max() < 2e-3


@pytest.mark.parametrize("ks", [7, 21, 33, 49, 65])
def test_render_fp16_arithmetic_stays_within_its_roundings_of_fp32(ks):
    """fp16 arithmetic against fp32 on the tiled (8, 4 and 2 pixels per tile), wave-per-pixel (ks 21 RGB, on a row of
    70 pixels: two chunks) and direct kernels, 1 / 3 / 4 channels: random kernels that sum to 1, image in [0,1)."""
    from sdirt_amd import local_dp_psf_render, local_psf_render_fast
    g = torch.Generator(device=DEV).manual_seed(ks)
    # Image value, weight, product and result are each rounded to fp16 once (relative 2^-11 each, outputs
    # <= 1), and a product below the fp16 normal range (weights ~ 1/ks^2 times values < 1) loses at most
    # half a subnormal step, 2^-25, ks^2 times.  Both paths add in fp32 in the same lane-strided order
    # (about ks^2/64 + 6 additions per partial sum, 2^-24 relative each: below 1e-5 at ks 65), which the
    # first term's slack over the 5e-4 measured on fixture f7 covers.
    bound = 4 * 2.0 ** -11 + ks * ks * 2.0 ** -25
    H, W = (5, 70) if ks == 21 else (5, 9)
    for C in (1, 3, 4):
        img = torch.rand(1, C, H, W, device=DEV, generator=g)
        psf = torch.rand(1, H, W, 2, ks, ks, device=DEV, generator=g)
        psf = psf / psf.sum((-1, -2), keepdim=True)
        full = local_dp_psf_render(img, psf, kernel_size=ks)
        half = torch.cat(local_psf_render_fast(img, psf, kernel_size=ks), dim=1)
        err = float((half - full).abs().max())
        print(f"ks {ks} C {C}: |half - fp32| max {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (ks, C, err)


@pytest.mark.parametrize("name", ["rf50mm", "rf35mm"])
def test_own_geometric_optics_against_reference_state(name):
    """calc_fov / paraxial pupils / refocus computed here (device traces + float64
    closed-form line intersections) vs the values the reference computed
    (tests/golden/lens_state_*.json).  The reference's pupil is itself only
    reproducible to ~1.3e-5 relative (fp32 lstsq), its refocus depends on the
    2048 random rays drawn -- from the same seed (torch.manual_seed(0), the CPU generator's stream reproduced draw
    for draw) the sensor lands on the reference's position exactly."""
    from sdirt_amd.psfnet import PSFNet
    st = load_state(name)
    torch.manual_seed(0)
    lens = PSFNet(os.path.join(DATA, f"{name}.json"), sensor_res=(512, 768), kernel_size=21,
                  device=DEV)
    assert lens.aper_idx == st["aper_idx"]
    ez, er = lens.entrance_pupil()
    xz, xr = lens.exit_pupil()
    print(name, "entrance pupil", (ez, er), "ref", (st["pupil_z"], st["pupil_r"]),
          "exit", (xz, xr), "ref", (st["exit_pupil_z"], st["exit_pupil_r"]))
    # reference estimator (fp32 lstsq on the host): the reference's own spread between two
    # identical calls is 1.3e-5 (entrance) / 2e-4 (exit) relative
    assert abs(ez - st["pupil_z"]) < 2e-3 and abs(er / st["pupil_r"] - 1) < 1e-4
    assert abs(xz - st["exit_pupil_z"]) < 5e-3 and abs(xr / st["exit_pupil_r"] - 1) < 1e-3
    # exact estimator: deterministic, agrees with the reference's to its fp32 bias (~1e-3)
    lens.pupil_method = "exact"
    lens._pupil_cache.clear()
    ez2, er2 = lens.entrance_pupil()
    assert abs(er2 / st["pupil_r"] - 1) < 3e-3 and abs(ez2 - st["pupil_z"]) < 5e-3
    lens.pupil_method = "reference"
    lens._pupil_cache.clear()
    lens.refocus(-1000 + lens.d_sensor)                       # 1_fit_psfnet.py:23-25
    m = dict(d_sensor=abs(lens.d_sensor - st["d_sensor"]), hfov=abs(lens.hfov / st["hfov"] - 1),
             foclen=abs(lens.foclen / st["foclen"] - 1), fnum=abs(lens.fnum / st["fnum"] - 1))
    print(name, "after refocus (seed 0): d_sensor", lens.d_sensor, "ref", st["d_sensor"], "MEASURED", m)
    # measured (MI355X box, EPYC host, torch 2.10 / numpy 2.2): 0.0 mm -- the reference's 62.25132751464844 /
    # 81.8495864868164 to the last fp32 digit -- and 0 / 0 / 8e-8 relative.  The bound leaves room for another host:
    # the result rests on the CPU generator's stream and on host-side fp reductions (np.mean, lstsq), which a
    # different CPU, torch build or BLAS may round differently with no defect in the product
    assert m["d_sensor"] < 1e-4
    assert m["hfov"] < 1e-4
    assert m["foclen"] < 1e-4
    assert m["fnum"] < 1e-4
    # with the sensor pinned to the reference's value hfov agrees tightly (same 100 rays)
    lens.d_sensor = st["d_sensor"]
    lens.post_computation()
    m2 = dict(hfov=abs(lens.hfov / st["hfov"] - 1), foclen=abs(lens.foclen / st["foclen"] - 1),
              fnum=abs(lens.fnum / st["fnum"] - 1))
    print(name, "sensor pinned: MEASURED", m2)
    assert m2["hfov"] < 1e-5 and m2["foclen"] < 1e-5 and m2["fnum"] < 1e-5


def test_psfnet_data_generators():
    from sdirt_amd.psfnet import PSFNet
    st = load_state("rf50mm")
    lens = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=21,
                  device=DEV)
    lens.set_state(d_sensor=st["d_sensor"], hfov=st["hfov"], pupil=(st["pupil_z"], st["pupil_r"]))
    torch.manual_seed(0); np.random.seed(0)
    inp, psf = lens.get_training_data(bs=64, spp=2048)       # training shape (1_fit_psfnet.py:36)
    assert inp.shape == (64, 3) and psf.shape == (64, 21, 21) and psf.is_cuda
    assert float(psf.amax((1, 2)).min()) > 0.999 and float(psf.min()) >= 0
    assert (inp[:, :2].abs() <= 1).all() and (inp[:, 2] >= 0).all() and (inp[:, 2] <= 1).all()
    # RNG order of the reference: choice, rand, rand, randn, then the PSF call's draws
    torch.manual_seed(0); np.random.seed(0)
    np.random.choice(lens.foc_z_arr)
    x = (torch.rand(64) - 0.5) * 2
    assert torch.equal(inp[:, 0], x)
    inp2, psf2 = lens.get_test_data(bs=1024, spp=256)
    assert inp2.shape == (1024, 3) and psf2.shape == (1024, 21, 21)
    assert float(lens.z2depth(torch.tensor(0.0))) == -200 and float(lens.z2depth(torch.tensor(1.0))) == -20000


def _psfnet_with_fixture_net(fx, prefix="w/"):
    from test_psfnet_cpu import make_psfnet, small_net
    m = make_psfnet(int(fx["ks"]), device=DEV)
    m.psfnet = small_net(fx, prefix).to(DEV)
    return m


def test_psfnet_pred_and_render_against_reference():
    """psfnet.py:317-336 and 642-714 on the f9 fixture (small seeded MLP, 8x12 image, ks 7).
    The reference values are its CPU fp32 results; on the GPU the network runs under fp16
    autocast as the reference does on CUDA (psfnet_arch.py:46), hence fp16 tolerances."""
    fx = load_golden("f9_psfnet_forward")
    m = _psfnet_with_fixture_net(fx)
    inp = t(fx["pred_inp"].copy())
    with torch.no_grad():
        psf = m.pred(inp)
    assert psf.shape == fx["pred"].shape
    assert torch.equal(inp[..., 0].cpu(), torch.from_numpy(-fx["pred_inp"][..., 0]))
    assert np.abs(psf.float().cpu().numpy() - fx["pred"]).max() < 2e-3 * fx["pred"].max()
    out = m.render(t(fx["img"]), t(fx["depth"]), t(fx["foc_dist"]))
    assert out.shape == fx["render"].shape and out.dtype == torch.float32
    # fp16 kernels and fp16 products in linear light, then the gamma curve (slope <= ~4 here)
    assert np.abs(out.cpu().numpy() - fx["render"]).max() < 4e-3
    assert np.abs(out.cpu().numpy() - fx["render"]).mean() < 5e-4
    # the fused flip + normalise + convolve kernel against the reference's op-by-op chain
    m.fused_render = False
    chained = m.render(t(fx["img"]), t(fx["depth"]), t(fx["foc_dist"]))
    m.fused_render = True
    assert (out - chained).abs().max().item() < 1.5e-3
    assert np.abs(chained.cpu().numpy() - fx["render"]).max() < 4e-3
    # fp32 network (autocast off) narrows the gap to the convolution's own fp16 rounding
    with torch.autocast("cuda", enabled=False):
        m.psfnet.forward = lambda x: m.psfnet.net(x).reshape(*x.shape[:-1], m.psfnet.ks, m.psfnet.ks)
        out32 = m.render(t(fx["img"]), t(fx["depth"]), t(fx["foc_dist"]))
    assert np.abs(out32.cpu().numpy() - fx["render"]).max() < 3e-3


def test_psfnet_fits_ray_traced_psfs_on_the_gpu(tmp_path):
    """train_psfnet (psfnet.py:101-168) end to end: batches come from the HIP PSF kernels,
    the loss of a small network drops, the checkpoint round-trips through load_net."""
    from sdirt_amd.psfnet import PSFNet
    from sdirt_amd.psfnet_arch import MLP, initialize_weights
    torch.manual_seed(0); np.random.seed(0)
    m = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=11, device=DEV)
    m.refocus(-1000 + m.d_sensor)
    m.psfnet = MLP(3, 121, hidden_features=128, hidden_layers=2).to(DEV)
    m.psfnet.apply(initialize_weights)
    losses = m.train_psfnet(iters=150, bs=64, lr=2e-3, spp=1024, evaluate_every=10 ** 6,
                            result_dir=str(tmp_path))
    assert len(losses) == 151 and np.isfinite(losses).all()
    assert np.mean(losses[-20:]) < 0.7 * np.mean(losses[:5])
    w = {k: v.clone() for k, v in m.psfnet.state_dict().items()}
    m.psfnet.apply(initialize_weights)
    m.load_net(str(tmp_path / "PSFNet_mlp.pkl"))
    assert all(torch.equal(w[k], v) for k, v in m.psfnet.state_dict().items())
    cmp = m.compare_psf(spp=4096, save_dir=str(tmp_path))
    assert set(cmp) == {-500, -20000}
    assert all(os.path.getsize(tmp_path / f"{kind}_{d}_{v}.png") > 1000
               for kind in ("rt", "pred") for d in (-500, -20000) for v in ("v00", "v04", "v08"))
    assert m.compare_psf(spp=1024, figures=False).keys() == cmp.keys()
    traced, predicted = cmp[-500]
    assert traced.shape == (3, 2, 11, 11) and predicted.shape == (3, 2, 11, 11)


def test_pipelined_training_loop_equals_the_plain_loop(tmp_path):
    """hipGraph-replayed forward/backward + fused AdamW + PSF batches prefetched on a second
    stream draw the same random numbers and take the same steps as the plain loop."""
    from sdirt_amd.psfnet import PSFNet
    from sdirt_amd.psfnet_arch import MLP, initialize_weights
    runs = []
    for pipelined in (False, True):
        torch.manual_seed(1); np.random.seed(1)
        m = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=11, device=DEV)
        m.refocus(-1000 + m.d_sensor)
        m.psfnet = MLP(3, 121, hidden_features=64, hidden_layers=2).to(DEV)
        m.psfnet.apply(initialize_weights)
        # evaluations (which draw the test set from the same CPU generators) fall INSIDE the run:
        # the prefetcher must not draw batch i+1 before evaluate(i) has drawn
        losses = m.train_psfnet(iters=30, bs=32, lr=1e-3, spp=512, evaluate_every=7,
                                result_dir=str(tmp_path), pipelined=pipelined)
        runs.append((np.asarray(losses), {k: v.clone() for k, v in m.psfnet.state_dict().items()},
                     float(torch.rand(1)), float(np.random.rand())))
    (la, wa, ta, na), (lb, wb, tb, nb) = runs
    assert ta == tb and na == nb                             # both generators end in the same state
    assert la.shape == lb.shape == (31,)
    assert la[0] == pytest.approx(lb[0], rel=1e-3)           # same first batch, same weights
    np.testing.assert_allclose(la, lb, rtol=0.05)            # fp16 GEMMs + fused vs foreach AdamW
    for k in wa:
        assert torch.allclose(wa[k], wb[k], atol=5e-3), k


@pytest.mark.parametrize("shape", [(1, 3, 40, 56, 21), (2, 1, 9, 13, 5), (1, 4, 7, 33, 9), (1, 3, 5, 7, 31)])
def test_psfnet_render_kernel_equals_pred_then_render(shape):
    """sdirt_psfnet_render on random raw outputs == stack / fliplr / normalise in torch (fp16,
    as PSFNet.pred does on the GPU) followed by the fp16 convolution kernel.  At ks 21, C 3 both sides run the same
    wave-per-pixel body (render_wave): the independent float64 reference is in tests/test_gpu_lattice.py."""
    from sdirt_amd.render_psf import local_psf_render_fast, psfnet_render
    B, C, H, W, ks = shape
    g = torch.Generator(device=DEV).manual_seed(ks)
    raw = torch.rand(2, B, H, W, ks, ks, device=DEV, generator=g).half()
    raw[0, 0, 0, 0] = 0                                               # dead kernel -> renders 0
    img = torch.rand(B, C, H, W, device=DEV, generator=g)
    rl, rr = psfnet_render(img, raw[0], raw[1], ks)
    psf = torch.stack((raw[0], torch.flip(raw[1], dims=[-1])), dim=-3).float()
    psf = psf / (psf.sum((-1, -2), keepdim=True).half().float() + 1e-9)
    el, er = local_psf_render_fast(img, psf.half(), kernel_size=ks)
    assert rl.shape == (B, C, H, W) and torch.isfinite(rl).all() and torch.isfinite(rr).all()
    assert rl[0, :, 0, 0].abs().max() == 0
    # identical arithmetic except reciprocal-multiply vs divide before the fp16 rounding of a tap
    assert (rl - el).abs().max().item() <= 1e-3 and (rr - er).abs().max().item() <= 1e-3
    assert ((rl == el).float().mean().item() > 0.7) and ((rr == er).float().mean().item() > 0.7)


def _emulate_autocast_mlp(net, x):
    """Linear + ReLU chain as fp16 autocast computes it: fp16 operands, fp32 sums, fp16 results."""
    h = x.half()
    for m in net.net:
        if isinstance(m, torch.nn.Linear):
            h = (h.float() @ m.weight.half().float().t() + m.bias.float())
        else:
            h = torch.relu(h).half()
    return h


@pytest.mark.parametrize("h4,layers,out,n", [(128, 8, 441, 1000), (32, 1, 25, 77), (64, 2, 512, 256),
                                              (96, 3, 121, 129)])
def test_fused_mlp_kernel_equals_the_layer_by_layer_network(h4, layers, out, n):
    """sdirt_psfnet_mlp (all layers in one kernel, activations in LDS, MFMA) against the same
    arithmetic done layer by layer in torch, with and without the mirrored second pass."""
    from sdirt_amd.psfnet_arch import MLP
    torch.manual_seed(h4 + n)
    net = MLP(3, out, hidden_features=512, hidden_layers=layers)
    net.net[0] = torch.nn.Linear(3, h4)
    net.net[2] = torch.nn.Linear(h4, 512)
    torch.nn.init.kaiming_uniform_(net.net[0].weight); torch.nn.init.kaiming_uniform_(net.net[2].weight)
    for m in net._linears():
        torch.nn.init.uniform_(m.bias, -0.1, 0.1)
    net = net.to(DEV)
    assert net.fused_supported()
    x = torch.rand(n, 3, device=DEV) * 2 - 1
    ref = _emulate_autocast_mlp(net, x).float()
    got = net.forward_fused(x).reshape(n, out).float()
    scale = ref.abs().max().item()
    assert scale > 0
    # same operands, same fp32 accumulation up to summation order: differences are single fp16
    # roundings of the activations, amplified through the layers
    assert (got - ref).abs().max().item() <= 4e-3 * scale, (got - ref).abs().max().item() / scale
    assert ((got - ref).abs() <= 1e-3 * scale).float().mean().item() > 0.999
    both = net.forward_fused(x, mirror=True).reshape(2, n, out).float()
    assert torch.equal(both[0], got)
    xm = x.clone(); xm[:, 0] = -xm[:, 0]
    assert torch.equal(both[1], net.forward_fused(xm).reshape(n, out).float())
    # and against the stock autocast forward (hipBLASLt): same tolerance class
    with torch.autocast("cuda", dtype=torch.float16):
        auto = net.net(x).float()
    assert (got - auto).abs().max().item() <= 4e-3 * scale
    # repacking follows weight updates
    with torch.no_grad():
        net.net[-2].bias.add_(1.0)
    assert (net.forward_fused(x).reshape(n, out).float() - got).abs().max().item() > 0.5


def test_pred_uses_the_fused_network_without_changing_results():
    """PSFNet.pred under no_grad goes through sdirt_psfnet_mlp for the reference's architecture;
    with gradients enabled it stays on the torch.nn layers; both agree to fp16 rounding."""
    from sdirt_amd.psfnet import PSFNet
    torch.manual_seed(3)
    m = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=21, device=DEV,
               post_computation=False)
    with torch.no_grad():
        m.psfnet.net[-2].bias.add_(0.05)
    inp = torch.rand(1, 6, 9, 3, device=DEV)
    inp[..., :2] = inp[..., :2] * 2 - 1
    a = m.pred(inp.clone())                                   # grad mode: torch.nn layers
    with torch.no_grad():
        b = m.pred(inp.clone())                               # fused kernel
        m.fused_mlp = False
        c = m.pred(inp.clone())
    assert a.shape == b.shape == (1, 6, 9, 2, 21, 21) and b.dtype == torch.float16
    scale = c.float().abs().max().item()
    assert (b.float() - c.float()).abs().max().item() < 1e-2 * scale
    assert (a.float() - c.float()).abs().max().item() < 1e-2 * scale


def test_tone_curve_kernels_equal_the_torch_chain():
    """sdirt_tone_curve against fit_degamma / fit_gamma evaluated op by op in torch on the GPU."""
    from sdirt_amd.psfnet import PSFNet
    m = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(512, 768), kernel_size=7, device=DEV,
               post_computation=False)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.rand(100000, device=DEV, generator=g)
    x[:4] = torch.tensor([0.0, 1.0, 100 / 255, 0.5], device=DEV)
    lin_ref = m.fit_degamma(x * 255.)
    lin = m.degamma(x)
    assert (lin - lin_ref).abs().max().item() <= 2e-6 * lin_ref.abs().max().item()
    assert (lin == lin_ref).float().mean().item() > 0.99
    back_ref = torch.clip(m.gamma(lin_ref), 0.0, 1.0)
    back = m._tone(lin_ref, 1)
    assert (back - back_ref).abs().max().item() <= 1e-6
    assert (back == back_ref).float().mean().item() > 0.99
    assert (back - x).abs().max().item() < 1e-2               # gamma ~ inverse of degamma (two blended fits)


def _eager_frame(m, net, img, depth, foc):
    with torch.no_grad():
        pair = m.render(img, depth, foc)
        with torch.autocast("cuda", dtype=torch.float16):
            return pair, net(pair[:, :3].contiguous(), pair[:, 3:].contiguous())


def test_config5_image_simulation_then_depth_network_in_one_chain():
    """BASELINE config 5 as ONE chain at its real size (2_dfdp_net.py:273-344 renders, :165-230 feeds
    the depth network): seeded synthetic RGB-D frame 512 x 768 -> PSFNet.render with the full-size
    MLP (3 -> 128 -> 512 x 9 -> 441, seeded weights: the reference's checkpoints are not in its
    repository) -> DfDPNet (YRStereonet_3D) under fp16 autocast, as Basenet.forward runs it.
    Asserted: shapes, finiteness, the fused render path == the op-by-op path, the autocast
    disparity == the fp32 module's on the same dual-pixel pair."""
    from sdirt_amd.psfnet import PSFNet
    from sdirt_amd.dfdp import DfDPNet
    H, W, ks = 512, 768, 21
    torch.manual_seed(0)
    np.random.seed(0)
    m = PSFNet(os.path.join(DATA, "rf50mm.json"), sensor_res=(H, W), kernel_size=ks, device=DEV)
    m.refocus(-1000 + m.d_sensor)
    assert [l.out_features for l in m.psfnet.net if hasattr(l, "out_features")] == [128] + [512] * 9 + [441]
    with torch.no_grad():
        m.psfnet.net[-2].bias.add_(0.02)          # untrained kernels must not vanish under the final ReLU
    g = torch.Generator(device=DEV).manual_seed(5)
    img = torch.rand(1, 3, H, W, device=DEV, generator=g)
    # a smooth depth map 0.5 ... 5 m (mm, negative towards the scene as the scripts pass it, :303)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=DEV), torch.linspace(0, 1, W, device=DEV), indexing="ij")
    depth = -(500 + 4500 * (0.5 + 0.5 * torch.sin(3 * xx + 2 * yy)) * (0.3 + 0.7 * yy)).reshape(1, 1, H, W)
    foc = torch.tensor([-1000.0], device=DEV)

    dp = m.render(img, depth, foc)                                   # fused MLP + fused convolution
    assert dp.shape == (1, 6, H, W) and dp.dtype == torch.float32
    assert torch.isfinite(dp).all() and float(dp.min()) >= 0 and float(dp.max()) <= 1
    assert float((dp[:, :3] - dp[:, 3:]).abs().max()) > 1e-3       # L and R views differ
    m.fused_mlp = m.fused_render = False
    dp_chain = m.render(img, depth, foc)                             # torch.nn layers, pred, local_psf_render_fast
    m.fused_mlp = m.fused_render = True
    d_render = float((dp - dp_chain).abs().max())

    torch.manual_seed(1)
    net = DfDPNet().to(DEV).eval()
    left, right = dp[:, :3].contiguous(), dp[:, 3:].contiguous()
    with torch.no_grad():
        disp32 = net(left, right)
        with torch.autocast("cuda", dtype=torch.float16):
            disp16 = net(left, right)
    assert disp32.shape[-2:] == (H, W) and disp16.shape == disp32.shape
    assert torch.isfinite(disp16.float()).all() and torch.isfinite(disp32).all()
    d_disp = float((disp16.float() - disp32).abs().max())
    print(f"config 5 chain: fused vs op-by-op render {d_render:.2e}; fp16-autocast vs fp32 disparity {d_disp:.2e} px")
    assert d_render <= 1.5e-3
    assert d_disp <= 5e-2

    # the whole frame captured once in a hipGraph (sdirt_amd.graphs.GraphedCall) and replayed: the same kernels on the same
    # buffers -- the simulated pair equals the eager call's, also after the static inputs were refreshed in place
    from sdirt_amd.graphs import GraphedCall

    def frame():
        with torch.no_grad():
            pair = m.render(img, depth, foc)
            with torch.autocast("cuda", dtype=torch.float16):
                return pair, net(pair[:, :3].contiguous(), pair[:, 3:].contiguous())
    graphed = GraphedCall(frame, warmup=2, device=DEV)
    pair_g, disp_g = graphed()
    torch.cuda.synchronize()
    assert torch.equal(pair_g, dp) and float((disp_g.float() - disp16.float()).abs().max()) <= 2e-3
    img2 = torch.rand(1, 3, H, W, device=DEV, generator=g)
    want_pair, want_disp = (t.clone() for t in _eager_frame(m, net, img2, depth, foc))
    img.copy_(img2)
    pair_g, disp_g = graphed()
    torch.cuda.synchronize()
    assert torch.equal(pair_g, want_pair) and float((disp_g.float() - want_disp.float()).abs().max()) <= 2e-3
    assert not torch.equal(want_pair, dp)
