"""local_dp_psf_render under autograd on the GPU: the two backward kernels of sdirt_render_grad.hip against the float64
restatement (tests/render_f64.py, which tests/test_render_grad_cpu.py holds against the reference's own autograd).

The bar, per gradient element: |kernel - float64| <= n 2^-23 sum|terms|, n = the number of terms of that element's sum
(C for a kernel gradient; 2 ks^2, more on the borders, for an image gradient) and sum|terms| the same sum on the
operands' magnitudes.  That is the worst-case bound of an fp32 sum of n rounded products in any order
(gamma_n with u = 2^-24, doubled): derived, not measured."""
import numpy as np
import pytest
import torch

from conftest import load_state, make_lens
from render_f64 import abs_terms_f64, grads_f64, render_f64, sampled_grad_img, sampled_grad_psf, term_counts

from sdirt_amd.render_psf import local_dp_psf_render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23


def operands(b, c, h, w, ks, seed=0, device="cpu"):
    gen = torch.Generator(device=device).manual_seed(seed)
    mk = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32, device=device)
    return mk(b, c, h, w), mk(b, h, w, 2, ks, ks), mk(b, 2 * c, h, w)


def kernel_grads(img, psf, G, ks, img_grad=True, psf_grad=True):
    a = img.to(DEV).detach().requires_grad_(img_grad)
    k = psf.to(DEV).detach().requires_grad_(psf_grad)
    out = local_dp_psf_render(a, k, ks)
    assert out.grad_fn is not None
    out.backward(G.to(DEV))
    return out.detach(), a.grad, k.grad


def check(tag, got, want, scale, n):
    got, want, scale = got.detach().cpu().double(), want.double(), scale.double()
    ratio = ((got - want).abs() / (n * EPS * scale).clamp_min(1e-300))
    print(f"{tag}: worst |kernel - float64| / (n 2^-23 sum|terms|) = {float(ratio.max()):.3f} "
          f"(n up to {int(torch.as_tensor(n).max())})")
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= n * EPS * scale).all()), (tag, float(ratio.max()))


# (B, C, H, W, ks): the specialised ks 21 RGB; ks 11 and 31 at sizes no tile divides; ks 63; one and four channels;
# a batch; an image smaller than the padding
CASES = [(1, 3, 48, 80, 21), (1, 3, 37, 53, 11), (1, 3, 41, 50, 31), (1, 3, 20, 27, 63), (1, 1, 19, 35, 21),
         (1, 4, 23, 18, 11), (2, 3, 17, 33, 21), (1, 3, 5, 9, 21)]


@pytest.mark.parametrize("case", CASES)
def test_both_gradients_against_the_float64_restatement(case):
    *shape, ks = case
    img, psf, G = operands(*shape, ks, seed=ks + shape[2])
    c = shape[1]
    _, dimg, dpsf = kernel_grads(img, psf, G, ks)
    assert dimg.shape == img.shape and dpsf.shape == psf.shape
    wimg, wpsf = grads_f64(img, psf, G[:, :c], G[:, c:], ks)
    simg, spsf = abs_terms_f64(img, psf, G[:, :c], G[:, c:], ks)
    check(f"{case} d psf", dpsf, wpsf, spsf, c)
    check(f"{case} d img", dimg, wimg, simg, term_counts(shape, ks))
    assert float(dimg.abs().max()) > 0 and float(dpsf.abs().max()) > 0


@pytest.mark.parametrize("side", [0, 1])
def test_upstream_zero_on_one_side(side):
    b, c, h, w, ks = 1, 3, 48, 80, 21
    img, psf, G = operands(b, c, h, w, ks, seed=5)
    G[:, side * c:(side + 1) * c] = 0
    _, dimg, dpsf = kernel_grads(img, psf, G, ks)
    wimg, wpsf = grads_f64(img, psf, G[:, :c], G[:, c:], ks)
    simg, spsf = abs_terms_f64(img, psf, G[:, :c], G[:, c:], ks)
    check("one side d psf", dpsf, wpsf, spsf, c)
    check("one side d img", dimg, wimg, simg, term_counts((b, c, h, w), ks))
    assert not dpsf[:, :, :, side].any() and dpsf[:, :, :, 1 - side].any()       # the silent side's kernels: exactly 0


@pytest.mark.parametrize("which", ["img", "psf"])
def test_only_the_operand_that_requires_a_gradient_gets_one(which):
    b, c, h, w, ks = 1, 3, 21, 30, 11
    img, psf, G = operands(b, c, h, w, ks, seed=6)
    a = img.to(DEV).requires_grad_(which == "img")
    k = psf.to(DEV).requires_grad_(which == "psf")
    local_dp_psf_render(a, k, ks).backward(G.to(DEV))
    wimg, wpsf = grads_f64(img, psf, G[:, :c], G[:, c:], ks)
    simg, spsf = abs_terms_f64(img, psf, G[:, :c], G[:, c:], ks)
    if which == "img":
        assert k.grad is None
        check("img only", a.grad, wimg, simg, term_counts((b, c, h, w), ks))
    else:
        assert a.grad is None
        check("psf only", k.grad, wpsf, spsf, c)


def test_forward_under_grad_is_bit_equal_to_the_forward_without():
    for case in [(1, 3, 48, 80, 21), (2, 4, 17, 33, 11), (1, 1, 5, 9, 21)]:
        *shape, ks = case
        img, psf, G = operands(*shape, ks, seed=7)
        out, _, _ = kernel_grads(img, psf, G, ks)
        with torch.no_grad():
            plain = local_dp_psf_render(img.to(DEV).requires_grad_(True), psf.to(DEV), ks)
        detached = local_dp_psf_render(img.to(DEV), psf.to(DEV), ks)
        assert plain.grad_fn is None and detached.grad_fn is None
        assert torch.equal(out, plain) and torch.equal(out, detached)


def test_two_backward_passes_are_bit_identical():
    for case in [(1, 3, 48, 80, 21), (2, 3, 37, 53, 31)]:
        *shape, ks = case
        img, psf, G = operands(*shape, ks, seed=8)
        first, second = kernel_grads(img, psf, G, ks), kernel_grads(img, psf, G, ks)
        assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])


def test_double_backward_is_refused():
    img, psf, G = operands(1, 3, 8, 8, 5, seed=9)
    a = img.to(DEV).requires_grad_(True)
    out = local_dp_psf_render(a, psf.to(DEV), 5)
    (g,) = torch.autograd.grad(out, a, G.to(DEV), create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_full_size_on_a_fixed_sample_of_each_gradient():
    """512 x 768 RGB, ks 21 (1.39 GB of kernels): 4096 elements of each gradient, drawn once from a seeded generator
    -- the image's four corners in all three channels among them -- against the direct float64 evaluation of the
    two gradient formulas (render_f64.sampled_grad_*; held against autograd by tests/test_render_grad_cpu.py)."""
    b, c, h, w, ks = 1, 3, 512, 768, 21
    img, psf, G = operands(b, c, h, w, ks, seed=10, device=DEV)
    _, dimg, dpsf = kernel_grads(img, psf, G, ks)
    gl, gr = G[:, :c], G[:, c:]
    gen = torch.Generator().manual_seed(11)
    pick = lambda n, count: torch.randint(0, n, (count,), generator=gen)
    idx = torch.stack([pick(n, 4096) for n in (b, h, w, 2, ks, ks)], 1).to(DEV)
    got = dpsf[tuple(idx.unbind(1))]
    check("full size d psf", got, sampled_grad_psf(img, gl, gr, ks, idx).cpu(),
          sampled_grad_psf(img, gl, gr, ks, idx, absolute=True).cpu(), c)
    corners = torch.tensor([[0, ch, v, u] for ch in range(c) for v in (0, h - 1) for u in (0, w - 1)])
    idx = torch.cat([corners, torch.stack([pick(n, 4096 - len(corners)) for n in (b, c, h, w)], 1)]).to(DEV)
    got = dimg[tuple(idx.unbind(1))]
    want, n = sampled_grad_img(psf, gl, gr, ks, idx)
    scale, _ = sampled_grad_img(psf, gl, gr, ks, idx, absolute=True)
    assert int(n.min()) < 2 * ks * ks < int(n.max())                 # window cut by the image's end; border folding
    check("full size d img", got, want.cpu(), scale.cpu(), n)


def test_gradient_reaches_the_dp_sensor_parameters_through_the_image_loss():
    """PSFs of the points of a 16 x 24 image -> per-side sum normalisation -> local_dp_psf_render -> MSE against a fixed
    image.  Route A: backward() through the new Function.  Route B: the restatement's float64 d loss / d psf on the
    detached PSFs, fed to torch.autograd.grad(psf, [h, f, w], grad_outputs=...).  Both routes run the same
    (deterministic, linear) splat backward, so theta_A - theta_B = sum_e J_e (g_A - g_B)_e with J = d psf / d theta,
    and

        |theta_A - theta_B| <= sum_e |J_e| (eps_e + 2^-24 |g_e|)                      (2^-24: g_B rounded to fp32)

    eps_e bounds the fp32 error of g_e = d loss / d psf_e, to first order, from the sums of magnitudes of the chain
    k = psf / s, out = render(img, k), loss = mean((out - target)^2), M = out.numel(), kk = ks^2:
        upstream  G = 2 (out - target) / M,   dG = (kk + 2) 2^-23 (2 / M) (render(|img|, k) + |target|)
                  (the forward's sum of kk products, the subtraction, the scaling)
        kernels   d_e = sum_c G_c P_c,        dd_e = C 2^-23 sum_c |G_c P_c| + sum_c dG_c |P_c|
        psf       g_e = (d_e - sum_t d_t k_t) / s,
                  eps_e = (dd_e + sum_t dd_t k_t) / s + 2 (kk + 4) 2^-23 (|d_e| + sum_t |d_t| k_t) / s
                  (the normalisation's backward: a sum of kk products, a subtraction, a division; and its forward's
                  rounding of s and k, which is where the factor 2 comes from)
    |J_e| is taken from central differences of psf_lr on the same pupil samples (step 2^-6 of the parameter)."""
    lens = make_lens("rf50mm", DEV, load_state("rf50mm"))
    H, W, ks, C = 16, 24, 21, 3
    kk = ks * ks
    ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, H), torch.linspace(-0.6, 0.6, W), indexing="ij")
    pts = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.full((H * W,), -1500.0)], 1)
    torch.manual_seed(3)
    with torch.no_grad():
        lens.psf_lr(pts, ks=ks, spp=4096)
    x2, y2, xc, yc = (t.clone() for t in lens.last_pupil_points)
    gen = torch.Generator().manual_seed(4)
    img, target = torch.rand((1, C, H, W), generator=gen), torch.rand((1, 2 * C, H, W), generator=gen)
    vals = (0.78, 1.44, 0.3)

    def psfs(dp):
        L, R = lens.psf_lr(pts, ks=ks, spp=4096, dp=(*dp, 0.5), pupil_xy=(x2, y2), center_pupil_xy=(xc, yc))
        return torch.stack((L, R), -3)                                           # [N, 2, ks, ks]

    theta = [torch.tensor(v, requires_grad=True) for v in vals]
    psf = psfs(theta)
    assert psf.grad_fn is not None
    k = psf / psf.sum((-1, -2), keepdim=True)
    out = local_dp_psf_render(img.to(DEV), k.reshape(1, H, W, 2, ks, ks), ks)
    loss = ((out - target.to(DEV)) ** 2).mean()
    # route B first (it keeps the graph), in float64 on the detached PSFs
    p64 = psf.detach().cpu().double().requires_grad_(True)
    s64 = p64.sum((-1, -2), keepdim=True)
    k64 = (p64 / s64).reshape(1, H, W, 2, ks, ks)
    l64, r64 = render_f64(img.double(), k64, ks)
    out64 = torch.cat([l64, r64], 1)
    ((out64 - target.double()) ** 2).mean().backward()
    g64 = p64.grad
    route_b = torch.autograd.grad(psf, theta, grad_outputs=g64.float().to(DEV), retain_graph=True)
    loss.backward()
    route_a = [t.grad for t in theta]
    # eps_e, from the restatement on magnitudes
    with torch.no_grad():
        M = out64.numel()
        kd, sd = k64.detach(), s64.detach()
        aimg = img.double().abs()
        a_out = torch.cat(render_f64(aimg, kd, ks), 1)
        G = 2 * (out64.detach() - target.double()) / M
        dG = (kk + 2) * EPS * (2 / M) * (a_out + target.double().abs())
    d = grads_f64(img, kd, G[:, :C], G[:, C:], ks)[1].reshape(p64.shape)
    d_abs = abs_terms_f64(img, kd, G[:, :C], G[:, C:], ks)[1].reshape(p64.shape)
    dd = C * EPS * d_abs + abs_terms_f64(img, kd, dG[:, :C], dG[:, C:], ks)[1].reshape(p64.shape)
    kn = kd.reshape(p64.shape)
    fold = lambda t: (t + (t * kn).sum((-1, -2), keepdim=True)) / sd
    eps = fold(dd) + 2 * (kk + 4) * EPS * fold(d.abs())
    weight = (eps + 2.0 ** -24 * g64.abs()).to(DEV)
    for i, name in enumerate("hfw"):
        step = 2.0 ** -6 * vals[i]
        with torch.no_grad():
            up, down = ([v + sgn * step if j == i else v for j, v in enumerate(vals)] for sgn in (1, -1))
            J = (psfs(up).double() - psfs(down).double()) / (2 * step)
        bound = float((J.abs() * weight).sum())
        a, b_ = float(route_a[i]), float(route_b[i])
        print(f"d loss / d {name}: through the Function {a:.9e}, through the float64 d psf {b_:.9e}, "
              f"|difference| {abs(a - b_):.3e}, bound {bound:.3e}")
        assert np.isfinite(a) and a != 0.0
        assert abs(a - b_) <= bound, (name, a, b_, bound)
