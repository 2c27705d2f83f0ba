"""The backward pass of the per-pixel dual-pixel PSF convolution without a GPU: the float64 restatement
(tests/render_f64.py) and its autograd gradients against the reference's own local_dp_psf_render run in float64, the
direct evaluation of the two gradient formulas against that autograd, and the C ABI of the two backward entries."""
import os
import re
import sys

import pytest
import torch

from render_f64 import abs_terms_f64, grads_f64, render_f64, sampled_grad_img, sampled_grad_psf, term_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, H, W, ks): RGB at the specialised size, one and four channels, a batch, an image smaller than the padding
CASES = [(1, 3, 12, 17, 21), (2, 1, 9, 7, 5), (1, 4, 6, 11, 11), (1, 3, 5, 9, 21), (1, 1, 1, 1, 3), (1, 3, 1, 8, 7)]


def operands(b, c, h, w, ks, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn((b, c, h, w), generator=gen, dtype=torch.float64),
            torch.randn((b, h, w, 2, ks, ks), generator=gen, dtype=torch.float64),
            torch.randn((b, c, h, w), generator=gen, dtype=torch.float64),
            torch.randn((b, c, h, w), generator=gen, dtype=torch.float64))


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")
@pytest.mark.parametrize("case", CASES)
def test_restatement_and_its_gradients_are_the_references_in_float64(case):
    """Both are float64 sums of the same terms: 1e-12 of the largest value."""
    sys.path.insert(0, ROOT)
    from oracle._refimport import import_reference
    import_reference()
    from deeplens.render_psf import local_dp_psf_render
    *shape, ks = case
    img, psf, gl, gr = operands(*shape, ks)
    a, k = img.clone().requires_grad_(True), psf.clone().requires_grad_(True)
    ref = local_dp_psf_render(a, k, kernel_size=ks)
    left, right = render_f64(img, psf, ks)
    c = shape[1]
    for got, want in ((left, ref[:, :c]), (right, ref[:, c:])):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    (torch.cat([gl, gr], 1) * ref).sum().backward()
    for got, want in zip(grads_f64(img, psf, gl, gr, ks), (a.grad, k.grad)):
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("case", CASES)
def test_direct_gradient_formulas_are_the_autograd_gradients(case):
    """sampled_grad_psf / sampled_grad_img at EVERY element, values, term magnitudes and term counts."""
    *shape, ks = case
    b, c, h, w = shape
    img, psf, gl, gr = operands(*shape, ks, seed=1)
    dimg, dpsf = grads_f64(img, psf, gl, gr, ks)
    aimg, apsf = abs_terms_f64(img, psf, gl, gr, ks)
    idx = torch.cartesian_prod(*[torch.arange(n) for n in (b, h, w, 2, ks, ks)])
    for absolute, want in ((False, dpsf), (True, apsf)):
        got = sampled_grad_psf(img, gl, gr, ks, idx, absolute).reshape(want.shape)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    idx = torch.cartesian_prod(*[torch.arange(n) for n in (b, c, h, w)]).reshape(-1, 4)
    counts = term_counts(shape, ks)
    for absolute, want in ((False, dimg), (True, aimg)):
        got, n = sampled_grad_img(psf, gl, gr, ks, idx, absolute)
        assert float((got.reshape(want.shape) - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert torch.equal(n.reshape(counts.shape).double(), counts)
    # every kernel value is used once per channel: the counts add up to 2 ks^2 per pixel and channel
    assert float(counts.sum()) == b * c * h * w * 2 * ks * ks


def test_backward_entries_are_declared_exported_and_cite_the_reference():
    from sdirt_amd import _lib
    names = ["sdirt_local_psf_render_grad_psf", "sdirt_local_psf_render_grad_img",
             "sdirt_local_psf_render_grad_img_workspace_bytes"]
    header = open(os.path.join(ROOT, "include", "sdirt_dp.h")).read()
    h = _lib.lib()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(h, name)
        comment = header[:header.index("int " + name if "bytes" not in name else "int64_t " + name)].rsplit("/*", 1)[1]
        assert re.search(r"render_psf\.py:\d+", comment), name
    assert h.sdirt_abi_version() == 4
    # the workspace: one halo of (16 + ks - 1)^2 positions per 16 x 16 tile and channel; refused shapes give -1
    assert h.sdirt_local_psf_render_grad_img_workspace_bytes(1, 3, 512, 768, 21) == 4 * 32 * 48 * 3 * 36 * 36
    assert h.sdirt_local_psf_render_grad_img_workspace_bytes(2, 4, 5, 9, 63) == 4 * 2 * 4 * 78 * 78
    assert h.sdirt_local_psf_render_grad_img_workspace_bytes(1, 3, 8, 8, 20) == -1
    assert h.sdirt_local_psf_render_grad_img_workspace_bytes(1, 3, 8, 8, 65) == -1


def test_calls_without_a_gradient_take_the_plain_path(monkeypatch):
    """local_dp_psf_render goes through the autograd Function only in grad mode with an operand that requires one."""
    import importlib
    render_psf = importlib.import_module("sdirt_amd.render_psf")      # sdirt_amd.render_psf the attribute is a function
    seen = []
    monkeypatch.setattr(render_psf, "_render", lambda i, p, ks, half: seen.append("plain") or (i, i))
    monkeypatch.setattr(render_psf._LocalDpPsfRender, "apply", lambda *a: seen.append("grad"))
    img, psf = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 2, 3, 3)
    render_psf.local_dp_psf_render(img, psf, 3)
    with torch.no_grad():
        render_psf.local_dp_psf_render(img.clone().requires_grad_(True), psf, 3)
    render_psf.local_dp_psf_render(img.clone().requires_grad_(True), psf, 3)
    render_psf.local_dp_psf_render(img, psf.clone().requires_grad_(True), 3)
    assert seen == ["plain", "plain", "grad", "grad"]
