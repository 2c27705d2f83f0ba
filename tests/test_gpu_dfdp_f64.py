"""The depth-network kernels of sdirt_amd/csrc/sdirt_dfdp.hip -- cost volume (planar, pixel-major, adjoint), window
average (planar, pixel-major), sdirt_bn_relu, sdirt_upsample_trilinear_ndhwc, sdirt_disparity_regression,
sdirt_tone_curve -- against the float64 restatements of tests/dfdp_f64.py, whose docstring carries the exactness
arguments and the derivation of every bound, and whose conditions tests/test_dfdp_f64_cpu.py checks.  On lattice inputs
the float64 answer rounded once where the kernel rounds is the only correct result: torch.equal.  Everywhere else the
tolerance is a derived bound, printed next to what was measured.  The references run in torch, in float64, on the GPU."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dfdp_f64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float16, torch.float32)
_id = lambda d: str(d).split(".")[-1]  # noqa: E731


def _abi():
    from sdirt_amd import _lib
    from sdirt_amd.basics import stream_ptr
    return _lib, _lib.lib(), stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _half(dt):
    return 1 if dt == torch.float16 else 0


def _vl(dt):
    return 8 if dt == torch.float16 else 4


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(got, want):
    """Equal as numbers AND in the sign of every zero (torch.equal alone takes -0.0 for +0.0)."""
    got, want = got.double(), want.double()
    return torch.equal(got, want) and torch.equal(torch.signbit(got), torch.signbit(want))


def _where(got, want):
    bad = (got.double() != want.double()).nonzero()
    return f"{len(bad)} of {want.numel()} differ, first at {bad[:4].tolist()}, largest {float((got.double() - want.double()).abs().max()):.4g}"


def _misaligned(x):
    """The same values in storage that starts one element past a 16-byte boundary (x's own strides kept)."""
    flat = torch.empty(x.numel() + 16, dtype=x.dtype, device=x.device)
    if x.dim() == 4 and not x.is_contiguous():
        B, Cn, H, W = x.shape
        v = flat[1:1 + x.numel()].view(B, H, W, Cn).permute(0, 3, 1, 2)
    else:
        v = flat[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 != 0 and v.stride() == x.stride()
    return v


def _guarded(n, dt, sentinel=-777.0, guard=4096):
    """A 16-byte-aligned slice of n elements in the middle of a sentinel-filled buffer -> (whole, slice, check)."""
    whole = torch.full((guard + n + guard,), sentinel, dtype=dt, device=DEV)
    out = whole[guard:guard + n]
    assert out.data_ptr() % 16 == 0

    def untouched():
        return bool((whole[:guard] == sentinel).all()) and bool((whole[guard + n:] == sentinel).all())
    return whole, out, untouched


# ---- cost volume ----------------------------------------------------------------------------------------------------
def _cv_inputs(n, shape, dt):
    x = R.special_values(R.lattice_values(100 + n, shape, 128)).to(DEV, dt)
    y = R.special_values(R.lattice_values(200 + n, shape, 128).flip(0)).to(DEV, dt)
    return x, y


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("d_max", R.CV_DMAX)
def test_cost_volume_every_form_is_the_gather_bit_for_bit(d_max, dt):
    """Planar, pixel-major in 16-byte groups, pixel-major element-wise (odd channel counts, and a misaligned slice of
    an aligned count) -- NaN, +-inf and -0.0 among the values, bit patterns compared; then the adjoint on lattice
    gradients against the float64 sum rounded once.  Odd d_max, and the narrowest width d_max // 2 + 1."""
    from sdirt_amd.dfdp import dp_cost_volume
    cl = torch.channels_last
    for n, shape in enumerate(R.cv_cases(d_max)):
        B, Cn, H, W = shape
        x, y = _cv_inputs(n, shape, dt)
        want = R.cost_volume_gather(x, y, d_max)
        got = dp_cost_volume(x, y, d_max)
        assert got.is_contiguous() and torch.equal(_bits(got), _bits(want)), ("planar", shape)
        xc, yc = x.contiguous(memory_format=cl), y.contiguous(memory_format=cl)
        forms = [("pixel-major", xc, yc)]
        if Cn % _vl(dt) == 0:
            forms += [("misaligned x", _misaligned(xc), yc), ("misaligned y", xc, _misaligned(yc))]
        for name, a, b in forms:
            got = dp_cost_volume(a, b, d_max)
            if Cn > 1 and H * W > 1:
                assert got.is_contiguous(memory_format=torch.channels_last_3d) and not got.is_contiguous(), (name, shape)
            assert torch.equal(_bits(got), _bits(want)), (name, shape)
        # adjoint
        g = R.lattice_grad(300 + n, want.shape).to(DEV)
        gx, gy, terms = R.cost_volume_adjoint_f64(g, d_max)
        assert terms * 16 < R.EXACT
        a = R.lattice_values(1, shape, 8).to(DEV, dt).requires_grad_()
        b = R.lattice_values(2, shape, 8).to(DEV, dt).requires_grad_()
        dp_cost_volume(a, b, d_max).backward(g.to(dt))
        assert a.grad.dtype == dt
        assert torch.equal(a.grad.double(), R.to_type(gx, dt).double()), ("gx", shape, _where(a.grad, R.to_type(gx, dt)))
        assert torch.equal(b.grad.double(), R.to_type(gy, dt).double()), ("gy", shape, _where(b.grad, R.to_type(gy, dt)))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_cost_volume_adjoint_rounds_once_where_fp16_rounds(dt):
    """d_max = 64 and gradients of one sign: sums of 128 .. 256, where fp16 no longer holds multiples of 2^-4 -- the sum
    is taken in fp32 and rounded once (ties to even), not rounded at every step."""
    from sdirt_amd.dfdp import dp_cost_volume
    B, Cn, H, W, d_max = R.CV_HOT
    g = R.lattice_grad(7, (B, 2 * Cn, d_max, H, W), hot=True).to(DEV)
    gx, gy, terms = R.cost_volume_adjoint_f64(g, d_max)
    assert terms * 16 <= 64 * 64 and float(gx.max()) > 128
    a = torch.zeros(B, Cn, H, W, device=DEV, dtype=dt).requires_grad_()
    b = torch.zeros(B, Cn, H, W, device=DEV, dtype=dt).requires_grad_()
    dp_cost_volume(a, b, d_max).backward(g.to(dt))
    if dt == torch.float16:
        assert not torch.equal(R.round_f16(gx), gx)
    assert torch.equal(a.grad.double(), R.to_type(gx, dt).double()), _where(a.grad, R.to_type(gx, dt))
    assert torch.equal(b.grad.double(), R.to_type(gy, dt).double()), _where(b.grad, R.to_type(gy, dt))


def test_cost_volume_refuses_a_shift_range_wider_than_the_image_and_writes_nothing():
    from sdirt_amd.dfdp import dp_cost_volume
    _lib, lib, st = _abi()
    for dt in DTYPES:
        for d_max, W in ((2, 1), (7, 3), (20, 10)):
            x = torch.ones(1, 8, 2, W, device=DEV, dtype=dt)
            with pytest.raises(_lib.SdirtError):
                dp_cost_volume(x, x, d_max)
            with pytest.raises(_lib.SdirtError):
                dp_cost_volume(x.contiguous(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last), d_max)
            n = 16 * d_max * 2 * W
            whole, out, untouched = _guarded(n, dt)
            for fn in (lib.sdirt_dp_cost_volume, lib.sdirt_dp_cost_volume_nhwc):
                assert fn(_p(x), _p(x), 1, 8, d_max, 2, W, _half(dt), _p(out), st) != 0
            torch.cuda.synchronize()
            assert bool((whole == -777.0).all())
            # one column more is accepted
            x1 = torch.ones(1, 8, 2, d_max // 2 + 1, device=DEV, dtype=dt)
            assert dp_cost_volume(x1, x1, d_max).shape == (1, 16, d_max, 2, d_max // 2 + 1)


# ---- window average -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("k", R.WA_K)
def test_window_average_planar_bit_for_bit(k, dt):
    """sdirt_avg_pool_windows at W = k, either side of 256 columns (the column loop's second trip) and OW = 257 (the
    output loop's); k % 4 in {0, 1, 2, 3}: the four-row main loop and its remainder together."""
    from sdirt_amd.dfdp import WindowAverage
    pool = WindowAverage((k, k), stride=(k, k))
    for W in R.wa_planar_widths(k):
        x = R.wa_values(W + k, (1, 3, 2 * k, W)).to(DEV)
        want, terms = R.window_average_f64(x, k, dt)
        assert terms < R.EXACT
        got = pool(x.to(dt))
        assert got.dtype == dt and got.shape == want.shape
        assert torch.equal(got.double(), want), (k, W, _where(got, want))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("Cn", R.WA_NHWC_C)
def test_window_average_pixel_major_bit_for_bit(Cn, dt):
    """sdirt_avg_pool_windows_nhwc at group counts 1, 3, 5, 6, 16, 32 and 256 (lanes = 1), k = 1 (lanes = 1) to 32.
    (2048 fp32 channels are more than 256 groups: WindowAverage re-lays the map and takes the planar kernel.)"""
    from sdirt_amd.dfdp import WindowAverage
    for k in R.WA_NHWC_K:
        H, W = (k, 2 * k) if Cn >= 1024 else (2 * k, 3 * k)
        x = R.wa_values(Cn + k, (2, Cn, H, W)).to(DEV)
        want, terms = R.window_average_f64(x, k, dt)
        assert terms < R.EXACT
        xc = x.to(dt).contiguous(memory_format=torch.channels_last)
        got = WindowAverage((k, k), stride=(k, k))(xc)
        assert got.dtype == dt and got.is_contiguous()
        assert torch.equal(got.double(), want), (Cn, k, _where(got, want))
        if Cn == 24:                                                   # a view that starts off a 16-byte boundary
            got = WindowAverage((k, k), stride=(k, k))(_misaligned(xc))
            assert torch.equal(got.double(), want), (Cn, k, "misaligned")


# ---- batch norm + ReLU ----------------------------------------------------------------------------------------------
def _bn_abi(x, outer, Cn, inner, tables, relu, dt):
    _lib, lib, st = _abi()
    t32 = [t.to(DEV, torch.float32).contiguous() for t in tables]
    return lib.sdirt_bn_relu(_p(x), outer, Cn, inner, *(_p(t) for t in t32), 1 if relu else 0, _half(dt), st)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bn_relu_planar_bit_for_bit(dt):
    """sdirt_bn_relu on [outer, C, inner] through the C ABI with lattice tables: inner a multiple of the vector length
    and not, inner / vl either side of 1024 (one and two chunks per plane), an aligned and a misaligned base."""
    vl = _vl(dt)
    Cn, outer = 5, 2
    tables = R.bn_lattice_tables(11, Cn)
    for inner in (vl, 3, 1023 * vl, 1024 * vl, 1025 * vl, 1024 * vl + 3, 1023, 1025):
        for relu in (True, False):
            x = R.lattice_values(inner + relu, (outer, Cn, inner), 256).to(DEV)
            want = R.to_type(R.bn_relu_f64(x, tables, relu)[0], dt)
            for mis in (False, True):
                got = _misaligned(x.to(dt)) if mis else x.to(dt)
                assert _bn_abi(got, outer, Cn, inner, tables, relu, dt) == 0
                assert _same(got, want), (inner, relu, mis, _where(got, want))
    assert bool(torch.signbit(want[:, 0]).any()) and float(want[:, 0].abs().max()) == 0       # -0.0 came through


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("Cn", R.BN_PIXEL_MAJOR_C)
def test_bn_relu_pixel_major_bit_for_bit(Cn, dt):
    """sdirt_bn_relu on [pixels, C]: one channel per thread (3, 5, 250; any misaligned base up to 256 channels), 16-byte
    groups (32 .. 2048), group counts that do not divide 256 (264 / 8 = 33)."""
    _lib, lib, st = _abi()
    vl = _vl(dt)
    tables = R.bn_lattice_tables(Cn, Cn)
    pixels = 77
    for relu in (True, False):
        x = R.lattice_values(Cn + relu, (pixels, Cn), 256).to(DEV)
        want = R.to_type(R.bn_relu_f64(x, tables, relu)[0], dt)
        got = x.to(dt)
        rc = _bn_abi(got, pixels, Cn, 1, tables, relu, dt)
        if Cn > 256 and (Cn % vl or Cn // vl > 256):
            assert rc != 0 and torch.equal(got.double(), x)           # refused, nothing written
            continue
        assert rc == 0 and _same(got, want), (Cn, relu, _where(got, want))
        got = _misaligned(x.to(dt))
        rc = _bn_abi(got, pixels, Cn, 1, tables, relu, dt)
        if Cn > 256:
            assert rc != 0 and torch.equal(got.double(), x)
        else:
            assert rc == 0 and _same(got, want), (Cn, relu, "misaligned", _where(got, want))


def _real_bn(Cn, dims, seed):
    g = torch.Generator().manual_seed(seed)
    bn = (nn.BatchNorm3d if dims == 5 else nn.BatchNorm2d)(Cn).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(Cn, generator=g)); bn.running_var.copy_(torch.rand(Cn, generator=g) * 3 + 0.1)
        bn.weight.copy_(torch.randn(Cn, generator=g)); bn.bias.copy_(torch.randn(Cn, generator=g))
    return bn.to(DEV)


def _bn_bound(x, bn, relu, dt):
    """float64 on _bn_tables' fp32 tables -> (reference, bound): 4 roundings on |gamma (x - mean) invstd| + |beta|,
    half an fp16 ulp where the result is rounded to fp16 (taken at the far end of the fp32 interval)."""
    from sdirt_amd.dfdp import _bn_tables
    ref, mag = R.bn_relu_f64(x.double(), _bn_tables(bn, x.device), relu)
    bound = R.gamma_n(4) * mag
    if dt == torch.float16:
        bound = bound + R.half_ulp(ref.abs() + bound)
    return ref, bound


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bn_relu_with_real_tables_within_the_derived_bound(dt):
    """_bn_relu_ with nn.BatchNorm tables on general values, planar and pixel-major, 4-D and 5-D."""
    from sdirt_amd.dfdp import _bn_relu_
    g = torch.Generator().manual_seed(3)
    for shape in ((2, 32, 6, 16, 24), (2, 32, 17, 24), (1, 5, 7, 9), (2, 3, 3, 5, 7), (1, 264, 5, 7)):
        bn = _real_bn(shape[1], len(shape), shape[1])
        for fmt in (torch.contiguous_format, torch.channels_last_3d if len(shape) == 5 else torch.channels_last):
            for relu in (True, False):
                x = (3 * torch.randn(shape, generator=g)).to(DEV, dt).contiguous(memory_format=fmt)
                ref, bound = _bn_bound(x, bn, relu, dt)
                with torch.no_grad():
                    got = _bn_relu_(x.clone(memory_format=torch.preserve_format), bn, relu)
                assert got.dtype == dt and got.stride() == x.stride()
                err = (got.double() - ref).abs()
                worst = int((err / bound).argmax())
                print(f"bn_relu {shape} {_id(dt)} {fmt} relu={relu}: |out - ref| {float(err.reshape(-1)[worst]):.3e} of {float(bound.reshape(-1)[worst]):.3e} allowed")
                assert bool((err <= bound).all()), (shape, fmt, relu)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bn_relu_misaligned_pixel_major_view_with_many_channels_takes_the_torch_ops(dt):
    """More than 256 channels pixel-major are only taken in 16-byte groups, which a view off a 16-byte boundary cannot
    have: _bn_relu_ must choose the torch ops for it (before anything is launched), as its docstring says."""
    from sdirt_amd.dfdp import _bn_relu_, _layout
    Cn = 264                                                          # 33 / 66 groups
    bn = _real_bn(Cn, 4, 9)
    g = torch.Generator().manual_seed(4)
    x = (3 * torch.randn((2, Cn, 3, 5), generator=g)).to(DEV, dt).contiguous(memory_format=torch.channels_last)
    xm = _misaligned(x)
    assert xm.is_contiguous(memory_format=torch.channels_last) and _layout(x) == (30, 1) and _layout(xm) is None
    for relu in (True, False):
        with torch.no_grad():
            want = F.relu(bn(xm)) if relu else bn(xm)
            got = _bn_relu_(xm, bn, relu)                             # (raised SdirtError before _layout looked at the address)
            assert torch.equal(got, want) and torch.equal(xm, x)
            ref, bound = _bn_bound(x, bn, relu, dt)
            aligned = _bn_relu_(x.clone(memory_format=torch.preserve_format), bn, relu)      # the kernel, on the aligned tensor
        assert bool(((aligned.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bn_relu_special_values(dt):
    """NaN, +-inf, -0.0 and results that underflow the tensor's type, with and without ReLU.  Against the restatement
    bit for bit (identity tables: the arithmetic is exact), and against torch's ops as numbers: NaN passes the clamp,
    -inf clamps to 0, a negative result never comes out as a negative number.  The kernel clamps BEFORE it rounds: a
    tiny negative value becomes +0, not the -0.0 that rounding first would leave."""
    from sdirt_amd.dfdp import _bn_relu_
    Cn = 8
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, -2.0 ** -20, 2.0 ** -20, -3.0, 5.0, 1.0, -1.0, 0.5] * 2)
    x = vals.view(1, 1, 2, 12).expand(1, Cn, 2, 12).contiguous()
    # channel 0 .. 3: identity; 4 .. 7: invstd 2^-12 (2^-20 -> 2^-32: below half of fp16's smallest subnormal)
    tables = (torch.zeros(Cn), torch.tensor([1.0] * 4 + [2.0 ** -12] * 4), torch.ones(Cn), torch.zeros(Cn))
    bn = nn.BatchNorm2d(Cn).eval()
    with torch.no_grad():
        bn.running_var.copy_(1 / tables[1].double() ** 2 - bn.eps)
    bn = bn.to(DEV)
    for fmt in (torch.contiguous_format, torch.channels_last):
        for relu in (True, False):
            xin = x.to(DEV, dt).contiguous(memory_format=fmt)
            got = xin.clone(memory_format=torch.preserve_format)
            outer, inner = (1, 24) if fmt == torch.contiguous_format else (24, 1)
            assert _bn_abi(got, outer, Cn, inner, tables, relu, dt) == 0
            want = R.to_type(R.bn_relu_f64(xin.double(), tables, relu)[0], dt)
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == 2 * Cn
            assert _same(got.nan_to_num(9.0), want.nan_to_num(9.0)), (fmt, relu)
            if relu:
                assert not bool((torch.signbit(got) & ~nan & (got != 0)).any())
                assert not bool(torch.signbit(got[:, 4:, :, 5]).any())                   # the tiny negative: +0
            with torch.no_grad():                                      # torch's own ops agree as numbers
                ref = (F.relu(bn(xin.float())) if relu else bn(xin.float())).to(dt)
                ours = _bn_relu_(xin.clone(memory_format=torch.preserve_format), bn, relu)
            assert torch.equal(torch.isnan(ours), torch.isnan(ref))
            assert torch.equal(torch.isinf(ours), torch.isinf(ref)) and torch.equal(ours.nan_to_num(9.0, 7.0, -7.0) > 0, ref.nan_to_num(9.0, 7.0, -7.0) > 0)


# ---- upsampling -----------------------------------------------------------------------------------------------------
def _upsample_abi(x5, size, dt, out=None, misalign=False):
    """x5 [B,C,D0,H0,W0] (values) -> the kernel's [B,C,D,H,W] through the C ABI on [B,D,H,W,C] storage."""
    _lib, lib, st = _abi()
    B, Cn = x5.shape[:2]
    xs = x5.to(dt).permute(0, 2, 3, 4, 1).contiguous()
    if misalign:
        xs = _misaligned(xs)
    if out is None:
        out = torch.empty((B,) + tuple(size) + (Cn,), dtype=dt, device=DEV)
    _lib.check(lib.sdirt_upsample_trilinear_ndhwc(_p(xs), B, Cn, *x5.shape[2:], *size, _half(dt), _p(out), st))
    return out.view((B,) + tuple(size) + (Cn,)).permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("Cn", R.UP_C)
def test_upsample_on_the_lattice_bit_for_bit(Cn, dt):
    """out = 2 in - 1 and 4 in - 3 per axis (weights 0, 1/4, 1/2, 3/4, 1), in 1 .. 5 mixed over the axes, wide
    (C 8, 64) and element-wise (C 1, 5; C 8, 64 from a misaligned input) forms."""
    for n, ins in enumerate(R.UP_IN):
        for f in (2, 4):
            size = tuple(f * i - (f - 1) for i in ins)
            x = R.lattice_values(10 * n + f + Cn, (2, Cn) + ins, 128).to(DEV)
            ref, mag = R.trilinear_f64(x, size, True)
            assert float(mag.max()) * 1024 < R.EXACT
            want = R.to_type(ref, dt)
            got = _upsample_abi(x, size, dt)
            assert torch.equal(got.double(), want.double()), (ins, size, _where(got, want))
            if Cn % _vl(dt) == 0:                                      # off a 16-byte boundary: element-wise
                got = _upsample_abi(x, size, dt, misalign=True)
                assert torch.equal(got.double(), want.double()), (ins, size, "misaligned", _where(got, want))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_upsample_production_ratio_within_the_derived_bound(dt):
    """out = 2 in (Conv2x._up2) and an arbitrary size through the ABI, general values: float64 on the kernel's own fp32
    weights, 6 roundings on sum|w x| (+ half an fp16 ulp)."""
    from sdirt_amd.dfdp import Conv2x
    conv2x = Conv2x(8, 8).to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    for shape, size in (((1, 64, 5, 8, 12), None), ((2, 8, 3, 5, 7), None), ((1, 5, 2, 3, 4), None), ((1, 4, 1, 6, 5), None),
                        ((1, 8, 3, 5, 7), (7, 6, 23)), ((1, 3, 2, 2, 3), (5, 1, 4))):
        x = torch.randn(shape, generator=g).to(DEV, dt)
        if size is None:
            size = tuple(2 * s for s in shape[2:])
            with torch.no_grad():
                got = conv2x._up2(x.contiguous(memory_format=torch.channels_last_3d))
            assert got.is_contiguous(memory_format=torch.channels_last_3d)
        else:
            got = _upsample_abi(x, size, dt)
        assert got.dtype == dt and got.shape == shape[:2] + size
        ref, mag = R.trilinear_f64(x.double(), size, True, R.lerp_f32)
        bound = R.gamma_n(6) * mag
        if dt == torch.float16:
            bound = bound + R.half_ulp(ref.abs() + bound)
        err = (got.double() - ref).abs()
        worst = int((err - bound).argmax())
        print(f"upsample {shape} -> {size} {_id(dt)}: |out - ref| {float(err.reshape(-1)[worst]):.3e} of {float(bound.reshape(-1)[worst]):.3e} allowed; largest {float(err.max()):.3e}")
        assert bool((err <= bound).all())


# ---- disparity regression -------------------------------------------------------------------------------------------
def _disp_abi(x, md, hw, dt):
    _lib, lib, st = _abi()
    B, D0, H0, W0 = x.shape
    xs = x.to(dt).contiguous()
    out = torch.empty((B, 1) + tuple(hw), dtype=torch.float32, device=DEV)
    _lib.check(lib.sdirt_disparity_regression(_p(xs), B, D0, H0, W0, md, hw[0], hw[1], _half(dt), _p(out), st))
    return out


def _check_disp(tag, got, r, md, exact):
    bound = R.disparity_bound(r, md, exact)
    err = (got.double() - r["disp"]).abs()
    worst = int((err / bound).argmax())
    print(f"disparity {tag}: |out - ref| {float(err.reshape(-1)[worst]):.3e} of {float(bound.reshape(-1)[worst]):.3e} allowed; "
          f"largest {float(err.max()):.3e}; peaked on {100 * float((r['pmax'] > 0.5).double().mean()):.0f} %")
    assert bool((err <= bound).all()), tag


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("case", R.DISP_DYADIC, ids=lambda c: "x".join(map(str, c)))
def test_disparity_regression_at_dyadic_ratios(case, dt):
    """Disp (in-plane x 4) on the lattice: exact softmin arguments, the bound (4 kappa + 2 D + 2) u sum p |s|."""
    from sdirt_amd.dfdp import Disp
    d_in, md, H0, W0 = case
    x = R.peaked_cost(sum(case), 2, d_in, H0, W0).to(DEV)
    r = R.disparity_f64(x, md, (4 * H0, 4 * W0))
    with torch.no_grad():
        got = Disp(md)(x.to(dt)[:, None])
    assert got.dtype == torch.float32 and got.shape == (2, 1, 4 * H0, 4 * W0)
    _check_disp(f"{case} {_id(dt)}", got, r, md, True)
    assert torch.equal(got, _disp_abi(x, md, (4 * H0, 4 * W0), dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("case", R.DISP_GENERAL, ids=lambda c: "x".join(map(str, c)))
def test_disparity_regression_at_general_ratios_and_values(case, dt):
    """Non-dyadic depth ratios (3 -> 5, 7 -> 13, 1 -> 4), odd in-plane sizes through the ABI, general values: float64 on
    the kernel's fp32 weights; the arguments of the softmin now carry the interpolation's rounding."""
    d_in, md, H0, W0 = case
    g = torch.Generator().manual_seed(sum(case))
    x = (2 * torch.randn((2, d_in, H0, W0), generator=g)).to(dt).to(DEV)
    for hw in ((4 * H0, 4 * W0), (3 * H0 + 1, 5 * W0 - 1)):
        r = R.disparity_f64(x.double(), md, hw, R.lerp_f32)
        _check_disp(f"{case} -> {hw} {_id(dt)}", _disp_abi(x, md, hw, dt), r, md, False)


# ---- tone curves ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1))
def test_tone_curves_within_the_running_bound_and_past_the_launch_cap(mode):
    """sdirt_tone_curve on 1 048 576 + 77 values (a partial second pass of its loop): 0, 1, the knee from both sides and a
    dense ramp, against float64 with the bound the op sequence gives at each input."""
    from sdirt_amd.psfnet import PSFNet
    assert R.partial_second_pass(R.TONE_N, R.CAP_16_BLOCKS * 256)
    x = R.tone_inputs(mode).to(DEV)
    got = PSFNet._tone(x, mode)
    ref, bound = R.tone_f64(x, mode)
    err = (got.double() - ref).abs()
    worst = int((err / bound.clamp(min=1e-300)).argmax())
    print(f"tone mode {mode}: |out - ref| {float(err[worst]):.3e} of {float(bound[worst]):.3e} allowed at x = {float(x[worst]):.6g}; "
          f"largest {float(err.max()):.3e}; tail {float(err[-77:].max()):.3e}")
    assert got.dtype == torch.float32 and bool((err <= bound).all())
    assert float(ref[-77:].abs().min()) > 0                            # the tail is not a row of zeros


# ---- the second pass of every grid-stride loop ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_cost_volume_planar_past_the_launch_cap(dt):
    from sdirt_amd.dfdp import dp_cost_volume
    B, Cn, D, H, W = 1, 32, 20, 96, 138
    assert R.partial_second_pass(B * 2 * Cn * D * H * ((W + 3) // 4), R.CAP_64) and W % 4
    x, y = _cv_inputs(1, (B, Cn, H, W), dt)
    assert torch.equal(_bits(dp_cost_volume(x, y, D)), _bits(R.cost_volume_gather(x, y, D)))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("wide", (True, False))
def test_cost_volume_pixel_major_past_the_launch_cap(wide, dt):
    from sdirt_amd.dfdp import dp_cost_volume
    vl = _vl(dt)
    B, Cn, D, H, W = (1, vl, 5, 77, 5461) if wide else (1, 3, 5, 53, 2647)
    assert R.partial_second_pass(B * D * H * W * (2 * Cn // (vl if wide else 1)), R.CAP_64)
    x, y = _cv_inputs(2, (B, Cn, H, W), dt)
    cl = torch.channels_last
    got = dp_cost_volume(x.contiguous(memory_format=cl), y.contiguous(memory_format=cl), D)
    assert got.is_contiguous(memory_format=torch.channels_last_3d)
    assert torch.equal(_bits(got), _bits(R.cost_volume_gather(x, y, D)))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_cost_volume_adjoint_past_the_launch_cap(dt):
    from sdirt_amd.dfdp import dp_cost_volume
    B, Cn, D, H, W = 1, 3, 4, 701, 999
    assert R.partial_second_pass(B * 2 * Cn * H * W, R.CAP_64)
    g = R.lattice_grad(5, (B, 2 * Cn, D, H, W)).to(DEV)
    gx, gy, _ = R.cost_volume_adjoint_f64(g, D)
    a = torch.zeros(B, Cn, H, W, device=DEV, dtype=dt).requires_grad_()
    b = torch.zeros(B, Cn, H, W, device=DEV, dtype=dt).requires_grad_()
    dp_cost_volume(a, b, D).backward(g.to(dt))
    assert torch.equal(a.grad.double(), R.to_type(gx, dt).double()) and torch.equal(b.grad.double(), R.to_type(gy, dt).double())
    assert float(gx[..., -1].abs().max()) > 0 and float(gy[0, -1, -1].abs().max()) > 0


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bn_relu_pixel_major_past_the_launch_cap(dt):
    """256 groups: one pixel per block pass, 4096 blocks at most -> 4096 + 77 pixels."""
    Cn, pixels = 256 * _vl(dt), R.CAP_16_BLOCKS + 77
    groups = Cn // _vl(dt)
    assert R.partial_second_pass(pixels, R.CAP_16_BLOCKS * (groups * (256 // groups) // groups))
    tables = R.bn_lattice_tables(3, Cn)
    x = R.lattice_values(8, (pixels, Cn), 256).to(DEV)
    want = R.to_type(R.bn_relu_f64(x, tables, True)[0], dt)
    got = x.to(dt)
    assert _bn_abi(got, pixels, Cn, 1, tables, True, dt) == 0
    assert _same(got, want), _where(got, want)


@pytest.mark.parametrize("dt,Cn", [(torch.float16, 8), (torch.float32, 4), (torch.float32, 1)], ids=("f16-wide", "f32-wide", "f32-elementwise"))
def test_upsample_past_the_launch_cap(dt, Cn):
    ins = (41, 65, 202)
    size = tuple(2 * i - 1 for i in ins)
    wide = Cn % _vl(dt) == 0
    assert R.partial_second_pass(size[0] * size[1] * size[2] * (Cn // _vl(dt) if wide else Cn), R.CAP_64)
    x = R.lattice_values(6, (1, Cn) + ins, 128).to(DEV)
    ref, _ = R.trilinear_f64(x, size, True)
    got = _upsample_abi(x, size, dt)
    assert torch.equal(got.double(), R.to_type(ref, dt).double()), _where(got, R.to_type(ref, dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_disparity_regression_past_the_launch_cap(dt):
    D0, md, H0, W0 = 2, 4, 512, 513
    hw = (4 * H0, 4 * W0)
    assert R.partial_second_pass(hw[0] * hw[1], R.CAP_64)
    x = R.peaked_cost(3, 1, D0, H0, W0).to(DEV)
    r = R.disparity_f64(x, md, hw)
    _check_disp(f"past the cap {_id(dt)}", _disp_abi(x, md, hw, dt), r, md, True)
    assert float(r["disp"][..., -1, :].abs().max()) > 0


# ---- guard bands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_vector_storing_kernels_write_inside_their_output_only(dt):
    """Pixel-major cost volume, sdirt_bn_relu in place (both layouts), upsampling and the pixel-major window average
    through the C ABI into a 16-byte-aligned slice of a sentinel-filled buffer: both guard bands stay untouched, the slice
    holds the result."""
    _lib, lib, st = _abi()
    vl = _vl(dt)
    # cost volume, [B, D, H, W, 2C]
    B, Cn, D, H, W = 1, vl, 5, 3, 7
    x, y = _cv_inputs(0, (B, Cn, H, W), dt)
    xs, ys = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
    whole, out, untouched = _guarded(B * D * H * W * 2 * Cn, dt)
    _lib.check(lib.sdirt_dp_cost_volume_nhwc(_p(xs), _p(ys), B, Cn, D, H, W, _half(dt), _p(out), st))
    torch.cuda.synchronize()
    assert untouched()
    assert torch.equal(_bits(out.view(B, D, H, W, 2 * Cn).permute(0, 4, 1, 2, 3)), _bits(R.cost_volume_gather(x, y, D)))
    # batch norm in place: pixel-major [77, 3 vl] and planar [2, 3, 5 vl]
    for outer, Cb, inner in ((77, 3 * vl, 1), (2, 3, 5 * vl)):
        tables = R.bn_lattice_tables(1, Cb)
        xv = R.lattice_values(2, (outer, Cb, inner), 256).to(DEV)
        whole, out, untouched = _guarded(xv.numel(), dt)
        out.copy_(xv.to(dt).view(-1))
        assert _bn_abi(out, outer, Cb, inner, tables, True, dt) == 0
        torch.cuda.synchronize()
        assert untouched()
        assert _same(out.view(outer, Cb, inner), R.to_type(R.bn_relu_f64(xv, tables, True)[0], dt))
    # upsampling, [B, D, H, W, C]
    ins, Cu = (2, 3, 2), 2 * vl
    size = tuple(2 * i - 1 for i in ins)
    xv = R.lattice_values(3, (1, Cu) + ins, 128).to(DEV)
    whole, out, untouched = _guarded(size[0] * size[1] * size[2] * Cu, dt)
    got = _upsample_abi(xv, size, dt, out=out)
    torch.cuda.synchronize()
    assert untouched()
    assert torch.equal(got.double(), R.to_type(R.trilinear_f64(xv, size, True)[0], dt).double())
    # window average, pixel-major in, planar out
    Bw, Cw, k = 2, 3 * vl, 2
    xv = R.wa_values(4, (Bw, Cw, 2 * k, 3 * k)).to(DEV)
    xs = xv.to(dt).permute(0, 2, 3, 1).contiguous()
    whole, out, untouched = _guarded(Bw * Cw * 2 * 3, dt)
    _lib.check(lib.sdirt_avg_pool_windows_nhwc(_p(xs), Bw, 2 * k, 3 * k, Cw, k, _half(dt), _p(out), st))
    torch.cuda.synchronize()
    assert untouched()
    assert torch.equal(out.view(Bw, Cw, 2, 3).double(), R.window_average_f64(xv, k, dt)[0])
