"""The lattice inputs and float64 restatements of tests/dfdp_f64.py checked on the reference alone (no GPU, no native
library): every restatement against the float64 torch op it stands for, every lattice condition its docstring names,
and every cap the GPU tests rely on (peaked softmin, ties, non-trivial bits)."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dfdp_f64 as R


# ---- cost volume ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_max", R.CV_DMAX + (R.CV_HOT[4],))
def test_cost_volume_gather_and_adjoint_equal_the_slice_assignments(d_max):
    from sdirt_amd.dfdp import _cost_volume_reference
    cases = [R.CV_HOT[:4]] if d_max == R.CV_HOT[4] else R.cv_cases(d_max)
    assert any(w == d_max // 2 + 1 for _, _, _, w in cases) or d_max == R.CV_HOT[4]
    for n, (B, C, H, W) in enumerate(cases):
        assert d_max // 2 < W
        hot = d_max == R.CV_HOT[4]
        x = R.special_values(R.lattice_values(100 + n, (B, C, H, W), 128))
        y = R.special_values(R.lattice_values(200 + n, (B, C, H, W), 128).flip(0))
        want = _cost_volume_reference(x, y, d_max)
        got = R.cost_volume_gather(x, y, d_max)
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (d_max, B, C, H, W)     # bit patterns
        for dt in (torch.float16, torch.float32):                      # the gather is a copy in every type
            assert torch.equal(R.cost_volume_gather(x.to(dt), y.to(dt), d_max).double().nan_to_num(7.0), want.nan_to_num(7.0))
        # the adjoint against autograd through the slice assignments
        g = R.lattice_grad(300 + n, want.shape, hot=hot)
        assert float(g.abs().max()) <= 4 and torch.equal(g * 16, (g * 16).round())
        assert torch.equal(g, g.half().double())                       # exact in fp16
        x1, y1 = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True), torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        _cost_volume_reference(x1, y1, d_max).backward(g)
        gx, gy, terms = R.cost_volume_adjoint_f64(g, d_max)
        assert torch.equal(gx, x1.grad) and torch.equal(gy, y1.grad)
        assert terms * 16 <= 64 * 64 < R.EXACT and d_max <= 64
        assert float(gx.abs().max()) > 0 and (C == 0 or float(gy.abs().max()) > 0)
        if hot:
            both = torch.cat((gx, gy))
            changed = float((R.round_f16(both) != both).double().mean())
            ties = float(((R.round_f16(both) - both).abs() == R.half_ulp(both)).double().mean())
            print(f"hot adjoint: largest sum {float(both.max()):.1f}, changed by the fp16 rounding {changed:.2f}, on ties {ties:.2f}")
            assert float(both.max()) > 128 and changed > 0.2 and ties > 0.1
            # ... where accumulating in fp16 gives another answer: the test can tell the two apart
            acc = torch.zeros_like(gx).half()
            for i in range(d_max):
                acc = (acc.float() + g[:, :C, i].float()).half()
            assert not torch.equal(acc.double(), R.round_f16(gx))


def test_cost_volume_gather_keeps_special_values():
    x = R.special_values(torch.ones(1, 2, 3, 5))
    assert int(torch.isnan(x).sum()) == 1 and int(torch.isinf(x).sum()) == 2 and int((torch.signbit(x) & (x == 0)).sum()) == 1
    got = R.cost_volume_gather(x, x.clone(), 5)
    assert int(torch.isnan(got).sum()) >= 2 and int((torch.signbit(got) & (got == 0)).sum()) >= 2


# ---- window average -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.WA_K)
def test_window_average_restatement(k):
    x = R.wa_values(k, (2, 3, 4 * k, 5 * k))
    assert float(x.abs().max()) <= 8 and torch.equal(x, x.half().double()) and torch.equal(x * 16, (x * 16).round())
    pool = nn.AvgPool2d((k, k), stride=(k, k))
    exact = pool(x)
    for dt in (torch.float16, torch.float32):
        got, terms = R.window_average_f64(x, k, dt)
        assert terms < R.EXACT and terms <= 32 * 32 * 128
        assert float(got.abs().max()) > 0
        ulp = R.half_ulp(exact) * 2 if dt == torch.float16 else exact.abs() * 2.0 ** -23
        # within one rounding to fp32 and one to T of the float64 mean; equal to the mean rounded once when k is 2^n
        assert bool(((got - exact).abs() <= ulp / 2 + exact.abs() * 2.0 ** -23).all())
        if k & (k - 1) == 0:
            assert torch.equal(got, exact.float().to(dt).double())
    if k >= 6:                                                        # (k <= 4: a mean of 16 values m/16 below 8 is an fp16 number)
        assert not torch.equal(R.window_average_f64(x, k, torch.float16)[0], exact)       # the rounding decides bits
    assert 257 * k <= 12288 and all(w % k == 0 for w in R.wa_planar_widths(k))
    assert max(R.wa_planar_widths(k)) > 256 and max(R.wa_planar_widths(k)) // k > 256
    # dividing after the cast to fp16 is another function on these inputs
    s = x.reshape(2, 3, 4, k, 5, k).sum((3, 5))
    if k in (6, 7):      # (sums above 64 need more than fp16's 11 bits; for k = 2^n rounding the sum IS rounding the mean)
        late = (s.half() / torch.tensor(k * k).half()).double()
        assert not torch.equal(late, R.window_average_f64(x, k, torch.float16)[0])
    if k & (k - 1):                                                   # (s / k^2 rounded once is not s * fp32(1 / k^2))
        late = (s.float() / (k * k)).double()
        assert not torch.equal(late, R.window_average_f64(x, k, torch.float32)[0])


def test_window_average_nhwc_group_counts():
    groups = {c // vl for c in R.WA_NHWC_C for vl in (8, 4) if c // vl <= 256}
    assert {1, 3, 5, 6, 16, 32, 256} <= groups
    lanes = {max(1, min(256 // (c // vl), k * k)) for c in R.WA_NHWC_C for vl in (8, 4) if c // vl <= 256 for k in R.WA_NHWC_K}
    assert 1 in lanes and 256 in lanes and any(256 % g for g in groups)


# ---- batch norm + ReLU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (5, 32, 264))
def test_bn_relu_lattice_and_restatement(C):
    tables = R.bn_lattice_tables(C, C)
    mean, invstd, gamma, beta = tables
    assert torch.equal(mean * 16, (mean * 16).round()) and float(mean.abs().max()) <= 16
    assert set(invstd.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}
    assert torch.equal(gamma * 4, (gamma * 4).round()) and float(gamma.abs().max()) <= 4
    assert torch.equal(beta * 16, (beta * 16).round()) and float(beta.abs().max()) <= 16
    assert float(gamma[0]) == 0 and bool(torch.signbit(beta[0])) and float(beta[0]) == 0
    x = R.lattice_values(C + 1, (3, C, 7, 11), 256)
    assert float(x.abs().max()) <= 16 and torch.equal(x, x.half().double())
    # every intermediate of gamma * (x - mean) * invstd + beta is an fp32 number
    sh = (1, -1, 1, 1)
    a = x - mean.view(sh)
    b = gamma.view(sh) * a
    c = b * invstd.view(sh)
    for t in (a, b, c, c + beta.view(sh)):
        assert torch.equal(t, t.float().double()) and float(t.abs().max()) * 256 < 2 ** 18
    for relu in (True, False):
        y, mag = R.bn_relu_f64(x, tables, relu)
        # nn.BatchNorm2d in float64 with the same tables (eps folded into the variance: invstd = 1 / sqrt(var + eps))
        bn = nn.BatchNorm2d(C).double().eval()
        with torch.no_grad():
            bn.running_mean.copy_(mean); bn.running_var.copy_(1 / invstd ** 2 - bn.eps)
            bn.weight.copy_(gamma); bn.bias.copy_(beta)
            want = bn(x)
            want = F.relu(want) if relu else want
        assert bool(((y - want).abs() <= 1e-12 * mag).all())
        assert float(y.abs().max()) < 65504
    y, _ = R.bn_relu_f64(x, tables, True)
    zero = y[:, 0]
    assert float(zero.abs().max()) == 0 and bool(torch.signbit(zero).any()) and not bool(torch.signbit(zero).all())
    h = R.round_f16(y)
    changed = float((h != y).double().mean())
    ties = float((((h - y).abs() == R.half_ulp(y)) & (h != y)).double().mean())
    print(f"bn lattice C {C}: fp16 rounding changes {changed:.2f} of the results, {ties:.3f} on ties; nonzero {float((y != 0).double().mean()):.2f}")
    assert changed > 0.02 and ties > 0.005 and float((y > 0).double().mean()) > 0.2


def test_bn_tables_are_close_to_float64():
    """_bn_tables' fp32 invstd against 1 / sqrt(var + eps) in float64: var + eps rounds once (half of it reaches the
    result), sqrt and the reciprocal once each on the CPU, two ulp each allowed for a device rsqrt: 5 u."""
    from sdirt_amd.dfdp import _bn_tables
    g = torch.Generator().manual_seed(5)
    bn = nn.BatchNorm2d(64).eval()
    with torch.no_grad():
        bn.running_var.copy_(torch.rand(64, generator=g) * 4 + 0.05)
        bn.running_mean.copy_(torch.randn(64, generator=g))
    mean, invstd, gamma, beta = _bn_tables(bn, torch.device("cpu"))
    ref = 1 / torch.sqrt(bn.running_var.double() + bn.eps)
    rel = float(((invstd.double() - ref).abs() / ref).max())
    print(f"invstd table vs float64: {rel / R.U24:.2f} u of 5 u")
    assert rel <= 5 * R.U24
    assert torch.equal(mean, bn.running_mean) and torch.equal(gamma, bn.weight.detach()) and torch.equal(beta, bn.bias.detach())


# ---- interpolation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", (True, False))
def test_interpolation_rules_exact_and_fp32(align):
    for inp, out in ((1, 1), (2, 3), (3, 5), (5, 9), (5, 17), (3, 6), (5, 10), (32, 64), (48, 96), (7, 13), (1, 4), (3, 5), (10, 20), (20, 20), (6, 24)):
        i0, i1, l0, l1, src = R.lerp_exact(out, inp, align)
        j0, j1, m0, m1, srcf = R.lerp_f32(out, inp, align)
        # three fp32 roundings of numbers below `in` without align_corners, two (scale, product) below in - 1 with
        bound = 2.0 ** -23 * (inp - 1) if align else 2.0 ** -22 * inp
        d = float(np.abs(src - srcf).max())
        assert d <= bound, (inp, out, d, bound)
        assert int(i1.max()) <= inp - 1 and int(j1.max()) <= inp - 1
        far = np.abs(src - np.round(src)) > bound                      # away from an integer the corner is the same
        assert np.array_equal(i0[far], j0[far]) and np.array_equal(i1[far], j1[far])
        dyadic = (align and (out == 2 * inp - 1 or out == 4 * inp - 3)) or (not align and out in (inp, 2 * inp, 4 * inp))
        if dyadic:
            assert np.array_equal(i0, j0) and np.array_equal(i1, j1) and np.array_equal(l1, m1) and np.array_equal(l0, m0)
            assert np.array_equal(l1 * 8, np.round(l1 * 8))


@pytest.mark.parametrize("align", (True, False))
def test_trilinear_restatement_equals_interpolate(align):
    for n, (ins, outs) in enumerate((((2, 3, 5), (3, 5, 9)), ((1, 2, 3), (1, 3, 9)), ((3, 5, 2), (6, 10, 4)), ((3, 1, 7), (5, 4, 13)))):
        x = R.lattice_values(n, (2, 3) + ins, 128)
        got, mag = R.trilinear_f64(x, outs, align)
        want = F.interpolate(x, outs, mode="trilinear", align_corners=align)
        assert bool(((got - want).abs() <= 1e-13 * mag + 1e-300).all()), (ins, outs)
        # with the fp32 weights the value moves by at most the weights' distance from the exact ones
        got32, _ = R.trilinear_f64(x, outs, align, R.lerp_f32)
        assert float((got32 - got).abs().max()) <= 3 * 2 * 2.0 ** -22 * max(ins) * 16


def test_upsample_lattice_is_exact_and_alive():
    for ins in R.UP_IN:
        for f in (2, 4):
            outs = tuple(f * i - (f - 1) for i in ins)
            x = R.lattice_values(sum(ins) + f, (1, 5) + ins, 128)
            got, mag = R.trilinear_f64(x, outs, True)
            assert torch.equal(got * 1024, (got * 1024).round()) and float(mag.max()) * 1024 < R.EXACT
            assert torch.equal(got, got.float().double()) and float(got.abs().max()) > 0
            for a, b in zip(R.lerp_exact(outs[2], ins[2], True)[2:4], R.lerp_f32(outs[2], ins[2], True)[2:4]):
                assert np.array_equal(a, b) and np.array_equal(a * 4, np.round(a * 4))
    x = R.lattice_values(9, (1, 64, 3, 5, 2), 128)
    got, _ = R.trilinear_f64(x, (9, 17, 5), True)
    assert float((R.round_f16(got) != got).double().mean()) > 0.01                    # fp16 rounding decides bits


# ---- disparity regression -------------------------------------------------------------------------------------------
def _disp_torch(x, maxdisp, hw):
    """The torch branch of Disp.forward, in the tensor's type, to any in-plane size."""
    v = F.interpolate(x[:, None], [maxdisp, hw[0], hw[1]], mode="trilinear", align_corners=False)
    p = F.softmin(torch.squeeze(v, 1), dim=1)
    shifts = torch.arange(-maxdisp // 2, maxdisp // 2).view(1, -1, 1, 1)
    return torch.sum(p * shifts, 1, keepdim=True)


@pytest.mark.parametrize("case", R.DISP_DYADIC + R.DISP_GENERAL, ids=lambda c: "x".join(map(str, c)))
def test_disparity_restatement(case):
    d_in, md, H0, W0 = case
    dyadic = case in R.DISP_DYADIC
    x = R.peaked_cost(sum(case), 2, d_in, H0, W0)
    assert float(x.abs().max()) <= 8 and torch.equal(x * 16, (x * 16).round())
    r = R.disparity_f64(x, md, (4 * H0, 4 * W0))
    want = _disp_torch(x, md, (4 * H0, 4 * W0))
    assert float((r["disp"] - want).abs().max()) <= 1e-12 * md
    assert d_in <= 32 and md <= 64
    peaked = float((r["pmax"] > 0.5).double().mean())
    print(f"disparity {case}: largest p > 0.5 on {100 * peaked:.0f} % of the pixels; disp in [{float(r['disp'].min()):.2f}, {float(r['disp'].max()):.2f}]")
    if dyadic:
        assert md in (d_in, 2 * d_in)
        v = r["v"]
        assert torch.equal(v * 4096, (v * 4096).round()) and float(r["R"].max()) * 4096 < 2 ** 17 and float(r["M"].max()) <= 8
        assert torch.equal(v, v.float().double())
        assert peaked > 0.6
        assert float(r["disp"].max() - r["disp"].min()) > 0.9 or H0 * W0 <= 2       # the planes decide the answer
    # the fp32 weights move the result by less than the general bound allows for
    r32 = R.disparity_f64(x, md, (4 * H0, 4 * W0), R.lerp_f32)
    if dyadic:
        assert torch.equal(r32["disp"], r["disp"])
    b = R.disparity_bound(r32, md, dyadic)
    assert float(b.max()) < 1e-3 and float(b.min()) > 0


def test_disparity_shifts_of_odd_counts():
    for md in (1, 4, 5, 7, 13, 20, 64):
        first = (-md) // 2
        assert torch.equal(torch.arange(first, first + md), torch.arange(-md // 2, md // 2))


# ---- tone curves ----------------------------------------------------------------------------------------------------
def test_tone_restatement_equals_fit_degamma_and_fit_gamma():
    from sdirt_amd.psfnet import PSFNet
    assert R.TONE_DECIMAL == (PSFNet._TONE_LO, PSFNet._TONE_HI)
    x = torch.linspace(0, 1, 4001, dtype=torch.float64)
    got, _ = R.tone_f64(x, 0, R.TONE_DECIMAL, f32_constants=False)
    want = PSFNet.fit_degamma(PSFNet, x * 255.0)
    assert float(((got - want).abs() / want.abs().clamp(min=1e-30)).max()) < 1e-12
    lum = want
    assert 1100 < float(lum.max()) < R.TONE_LUM_MAX
    got, _ = R.tone_f64(lum, 1, R.TONE_DECIMAL, f32_constants=False)
    back = torch.clip(PSFNet.fit_gamma(PSFNet, lum) / 255.0, 0, 1)
    assert float((got - back).abs().max()) < 1e-12
    assert float((back - x).abs().max()) < 1e-2                       # the two curves are near inverses


@pytest.mark.parametrize("mode", (0, 1))
def test_tone_inputs_and_bound(mode):
    x = R.tone_inputs(mode, 20000)
    assert x.dtype == torch.float32 and float(x[0]) == 0 and float(x[1]) == 1 and float(x.min()) >= 0 and float(x.max()) == (1 if mode == 0 else R.TONE_LUM_MAX)
    knee = x[2:11].double()
    if mode == 0:
        assert float(knee[4]) == float(np.float32(100 / 255)) and float(knee[0] * 255) < 100 < float(knee[-1] * 255)
    else:
        t = R.tone_f64(knee, 1, blend=True)[0]
        assert float(t[0]) < 1 < float(t[-1])
    val, bound = R.tone_f64(x, mode)
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(bound).all())
    rel = bound / val.abs().clamp(min=2.0 ** -20)
    print(f"tone mode {mode}: bound up to {float(bound.max()):.2e} absolute, {float(rel.max()) / R.U24:.1f} u relative")
    assert float(bound.max()) < 1e-5 * (float(val.abs().max()) + 1)
    # the fp32 op sequence on the CPU (IEEE) stays inside its bound
    f = torch.float32
    (a1, b1, c1), (a2, b2, c2) = (tuple(torch.tensor(c, dtype=f) for c in row) for row in R.TONE_F32)
    one = torch.tensor(1.0, dtype=f)
    if mode == 0:
        v = x * 255.0
        lo, hi = one / (one / (a1 * v + b1) + c1), one / (one / (a2 * v + b2) + c2)
        t = torch.clamp(v * (one / 100), max=1)
        got = hi * t + lo * (1 - t)
    else:
        r = one / (x + torch.tensor(1e-9, dtype=f))
        x1, x2 = (one / (r - c1) - b1) * (one / a1), (one / (r - c2) - b2) * (one / a2)
        t = torch.clamp(((x1 + x2) * 0.5) * (one / 100), max=1)
        got = ((x2 * t + x1 * (1 - t)) * (one / 255)).clamp(0, 1)
    assert bool(((got.double() - val).abs() <= bound).all())


# ---- launch caps ------------------------------------------------------------------------------------------------------
def test_tone_count_enters_a_partial_second_pass():
    assert R.partial_second_pass(R.TONE_N, R.CAP_16_BLOCKS * 256) and R.TONE_N == 1048576 + 77
