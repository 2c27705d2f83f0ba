"""Ray-traced rendering of a textured plane, the parts that need no GPU: the C entry and its binding,
the float64 restatement of the lookup and the sums on landings made by hand, the upright condition of the lookup's
signs, and the argument errors of render_plane / render_single_img / sample_sensor."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_lens

ENTRY = "sdirt_render_plane"


def test_header_declares_the_entry_and_the_library_exports_it():
    import ctypes as C
    from sdirt_amd import _lib
    txt = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, code)
    assert "optics.py:497-538, 630-635, 756-780" in txt
    assert "#define SDIRT_ABI_VERSION 4" in txt
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    n_args = len(re.search(r"int\s+%s\s*\((.*?)\);" % ENTRY, code, re.S).group(1).split(","))
    assert restype is C.c_int and len(argtypes) == n_args == 24
    h = _lib.lib()
    assert hasattr(h, ENTRY)
    assert _lib.ABI_VERSION == 4 and h.sdirt_abi_version() == 4
    # a null lens is refused before anything touches a device
    assert h.sdirt_render_plane(None, None, 0, None, None, 0.0, None, None, 0.0, 1, 1, 1, None, -1.0, 1.0, None, 1, 1, 1,
                                None, None, None, None, None) != 0
    assert b"null lens" in h.sdirt_last_error()


def _landing(rays, H=1, W=1):
    """[5, S, H, W] from a list of (px, py, ra, w_L, w_R), the same S rays for every pixel."""
    a = torch.tensor(rays, dtype=torch.float32).t().reshape(5, len(rays), 1, 1)
    return a.expand(5, len(rays), H, W).contiguous()


TEX = torch.tensor([[[1.0, 2.0], [4.0, 8.0]], [[-1.0, 0.5], [0.25, 3.0]]])      # [T = 2, 2, 2]


def test_ray_at_the_common_corner_gives_the_mean_of_the_four_texels():
    from sdirt_amd.render_rt import images_from_sums, plane_sums_float64
    num, den = plane_sums_float64(_landing([(0.0, 0.0, 1.0, 0.5, 0.25)]), TEX, 1.0)
    assert num.dtype == den.dtype == torch.float64 and num.shape == (2, 2, 1, 1) and den.shape == (2, 1, 1)
    assert den.flatten().tolist() == [0.5, 0.25]
    assert num[:, :, 0, 0].tolist() == [[0.5 * 3.75, 0.5 * 0.6875], [0.25 * 3.75, 0.25 * 0.6875]]
    img = images_from_sums(num, den)
    assert img[:, :, 0, 0].tolist() == [[3.75, 0.6875], [3.75, 0.6875]]
    # one view: row 3 alone
    num1, den1 = plane_sums_float64(_landing([(0.0, 0.0, 1.0, 1.0, 1.0)]), TEX, 1.0, views=1)
    assert num1.shape == (1, 2, 1, 1) and num1.flatten().tolist() == [3.75, 0.6875] and den1.item() == 1.0


@pytest.mark.parametrize("px, py, want", [(1e4, 1e4, 4.0), (-1e4, 1e4, 8.0), (1e4, -1e4, 1.0), (-1e4, -1e4, 2.0),
                                          (3e38, 0.75, 4.0), (-0.25, -3e38, 0.25 * 1.0 + 0.75 * 2.0)])
def test_ray_far_outside_gives_the_clamped_corner_texel(px, py, want):
    """u = Wt / 2 - px inv, v = Ht / 2 + py inv: +x on the plane is the texture's LEFT and +y its BOTTOM -- the lens
    inverts, the rendered image is upright -- with replicate addressing beyond the texture."""
    from sdirt_amd.render_rt import plane_sums_float64
    num, den = plane_sums_float64(_landing([(px, py, 1.0, 1.0, 1.0)]), TEX[:1], 1.0)
    assert num[0, 0, 0, 0].item() == want and den[0, 0, 0].item() == 1.0


def test_dead_rays_contribute_to_neither_sum_and_an_all_dead_pixel_is_zero():
    from sdirt_amd.render_rt import images_from_sums, plane_sums_float64
    nan = float("nan")
    live = (0.0, 0.0, 1.0, 0.5, 0.25)
    for dead in [(0.3, -0.2, 0.0, 0.7, 0.9), (nan, nan, 0.0, 0.7, 0.9), (float("inf"), 1e30, 0.0, nan, 0.9)]:
        num, den, ab = plane_sums_float64(_landing([dead, live, dead]), TEX, 1.0, return_abs=True)
        one, den1 = plane_sums_float64(_landing([live]), TEX, 1.0)
        assert torch.equal(num, one) and torch.equal(den, den1) and torch.equal(ab, one.abs())
        num, den = plane_sums_float64(_landing([dead, dead]), TEX, 1.0)
        assert not num.any() and not den.any()
        img = images_from_sums(num, den)
        assert img.shape == num.shape and not img.any() and not img.isnan().any()
        assert not images_from_sums(num, den, spp=2, photometric=True).any()
    # photometric: num / spp whatever den is
    num, den = plane_sums_float64(_landing([live, (0.0, 0.0, 0.0, 1.0, 1.0)]), TEX, 1.0)
    assert images_from_sums(num, den, spp=2, photometric=True)[0, 0, 0, 0].item() == 0.5 * 3.75 / 2


def test_the_lookup_is_upright():
    """A ray from the centre (xs, ys) of sensor pixel (i, j) that lands at (-scale xs, -scale ys) -- where an ideal
    inverting lens of magnification 1 / scale puts it -- reads exactly tex[i, j].  Powers of two throughout (pixel
    2^-4 mm, scale 8, an 8 x 16 sensor), so every fp32 operation of the lookup is exact and `exactly` means bits."""
    from sdirt_amd.render_rt import plane_sums_float64
    H, W, ps, scale = 8, 16, 0.0625, 8.0
    xs = -W * ps / 2 + (torch.arange(W, dtype=torch.float32) + 0.5) * ps
    ys = H * ps / 2 - (torch.arange(H, dtype=torch.float32) + 0.5) * ps
    land = torch.zeros(5, 1, H, W)
    land[0, 0] = (-scale * xs)[None, :].expand(H, W)
    land[1, 0] = (-scale * ys)[:, None].expand(H, W)
    land[2:] = 1.0
    tex = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1))
    num, den = plane_sums_float64(land, tex, 1.0 / (scale * ps * W / W), views=1)
    assert torch.equal(num[0], tex.double()) and torch.equal(den[0], torch.ones(H, W, dtype=torch.float64))
    # a texture of twice the sensor's resolution: the pixel centre is the common corner of a 2 x 2 block of texels
    tex2 = torch.rand(1, 2 * H, 2 * W, generator=torch.Generator().manual_seed(2))
    num2, _ = plane_sums_float64(land, tex2, 1.0 / (scale * ps * W / (2 * W)), views=1)
    block = tex2.double().view(1, H, 2, W, 2)
    want = 0.25 * block[:, :, 0, :, 0] + 0.25 * block[:, :, 0, :, 1] + 0.25 * block[:, :, 1, :, 0] + 0.25 * block[:, :, 1, :, 1]
    assert torch.equal(num2[0], want)


def test_render_plane_refuses_bad_arguments_before_anything_touches_the_gpu():
    from sdirt_amd import _lib
    lens = make_lens("rf50mm", "cpu")
    lens.prepare_sensor(sensor_res=(4, 6), sensor_size=(1.0, 1.5))
    img = torch.zeros(1, 3, 4, 6)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        lens.render_plane(img[0], -1000.0, scale=10.0)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        lens.render_plane(img.numpy(), -1000.0, scale=10.0)
    with pytest.raises(ValueError, match="float32"):
        lens.render_plane(img.double(), -1000.0, scale=10.0)
    with pytest.raises(ValueError, match="2 wavelengths for an image of 3 channels"):
        lens.render_plane(img, -1000.0, wvln=[0.656, 0.486], scale=10.0)
    for spp in (0, -3):
        with pytest.raises(ValueError, match="spp must be at least 1"):
            lens.render_plane(img, -1000.0, spp=spp, scale=10.0)
    with pytest.raises(ValueError, match="img is on meta, the lens on cpu"):
        lens.render_plane(torch.zeros(1, 3, 4, 6, device="meta"), -1000.0, scale=10.0)
    with pytest.raises(ValueError, match="pupil_points"):
        lens.render_plane(img, -1000.0, spp=2, scale=10.0, pupil_points=(torch.zeros(2, 4, 6), torch.zeros(3, 4, 6)))
    # every argument in order: the call gets as far as asking for the GPU, which a CPU lens does not have
    with pytest.raises(_lib.SdirtError, match="GPU only"):
        lens.render_plane(img, -1000.0, spp=2, scale=10.0, pupil_points=(torch.zeros(2, 4, 6), torch.zeros(2, 4, 6)))


def test_render_single_img_and_sample_sensor_keep_the_reference_s_refusals():
    lens = make_lens("rf50mm", "cpu")
    before = (lens.sensor_res, lens.sensor_size, lens.pixel_size, lens.r_last)
    with pytest.raises(Exception, match="This function only supports ndarray input. If you want to render an image batch, "
                                        "use `render` function."):
        lens.render_single_img(torch.zeros(16, 24, 3))
    with pytest.raises(Exception, match="Monochrome image is not tested yet."):
        lens.render_single_img(np.zeros((16, 24), np.uint8))
    with pytest.raises(AssertionError, match="Only support RGB image"):
        lens.render_single_img(np.zeros((16, 24, 4), np.uint8))
    with pytest.raises(NotImplementedError, match="unwarp"):
        lens.render_single_img(np.zeros((16, 24, 3), np.uint8), unwarp=True)
    assert (lens.sensor_res, lens.sensor_size, lens.pixel_size, lens.r_last) == before
    # an image that is not 2:3 fails prepare_sensor's square-pixel assertion AFTER it has assigned: the sensor is put back
    with pytest.raises(AssertionError, match="Pixel is not square"):
        lens.render_single_img(np.zeros((16, 16, 3), np.uint8), method="raytracing")
    assert (lens.sensor_res, lens.sensor_size, lens.pixel_size, lens.r_last) == before
    with pytest.raises(Exception, match="This feature has been abandoned."):
        lens.sample_sensor(pupil=False)
    with pytest.raises(Warning, match="This feature is not finished yet."):
        lens.sample_sensor(sub_pixel=True)


def test_sensor_axes_are_sample_sensor_s_corners_and_the_pixel_centres():
    from sdirt_amd.render_rt import sensor_axes
    lens = make_lens("rf50mm", "cpu")
    lens.prepare_sensor(sensor_res=(4, 6), sensor_size=(1.0, 1.5))
    x1, y1 = sensor_axes(lens)
    assert x1.dtype == torch.float32 and x1.tolist() == [-0.5, -0.25, 0.0, 0.25, 0.5, 0.75]
    assert y1.tolist() == [0.25, 0.0, -0.25, -0.5]
    xc, yc = sensor_axes(lens, pixel_center=True)
    assert xc.tolist() == [-0.625, -0.375, -0.125, 0.125, 0.375, 0.625] and yc.tolist() == [0.375, 0.125, -0.125, -0.375]
