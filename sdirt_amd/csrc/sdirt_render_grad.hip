// sdirt_render_grad.hip -- backward pass of the fp32 per-pixel dual-pixel PSF convolution of libsdirt_dp.so
// (MI355X / gfx950 only): local_dp_psf_render (deeplens/render_psf.py:157-188) under autograd, the gradients with
// respect to the per-pixel kernels and to the image.  The forward is sdirt_local_psf_render (sdirt_render.hip).
//
// P = replicate-padded image, pad = (ks - 1) / 2.  Tap (i, j) of the stored kernel of pixel (y, x) multiplies
// P[y + ks-1-i, x + ks-1-j] = img[clamp(y + pad - i), clamp(x + pad - j)] (the flip of render_psf.py:175).
//   dK  [b,y,x,s,i,j] = sum_c G_s[b,c,y,x] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)]
//   dImg[b,c,v,u]     = sum_s sum_{(y,x,i,j): clamp(y+pad-i) = v, clamp(x+pad-j) = u} G_s[b,c,y,x] * K[b,y,x,s,i,j]
// fp32 operands and sums, no atomics: every sum is taken by one thread in a fixed order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/sdirt_dp.h"
#include "sdirt_device.hpp"
#include "sdirt_host.hpp"
#include "sdirt_render.hpp"

using namespace sdirt;

// ---------------------------------------------------------------------------
// gradient with respect to the kernels
// ---------------------------------------------------------------------------
// One WAVE per pixel, as the forward: its 2*ks*ks gradients are one contiguous run of the output, which the lanes
// write as (64 / ks) whole kernel rows per step -- consecutive lanes, consecutive addresses, every value written
// once with a streaming store.  The 2C upstream values of the pixel are wave-uniform; the image (a few MB) is
// gathered through L1 / L2 at the clamped coordinates.  A workgroup of 4 waves covers kGradChunk pixels of a row.
constexpr int kGradChunk = 16;

template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_grad_psf(const float* __restrict__ img, const float* __restrict__ gl, const float* __restrict__ gr, int H,
                  int W, int ks, float* __restrict__ dk)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.y, b = blockIdx.z;
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ img_b = img + (int64_t)b * C * HW;
    const int rows_per_iter = 64 / ks;                                // ks <= 64 on this path
    const int row = lane / ks, col = lane - row * ks;
    const bool lane_on = row < rows_per_iter;
    const int x_end = min(W, ((int)blockIdx.x + 1) * kGradChunk);
    for (int x = blockIdx.x * kGradChunk + wave; x < x_end; x += kBlock / 64) {
        const int64_t o = ((int64_t)b * C * H + y) * W + x;
        float ul[C], ur[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { ul[c] = gl[o + c * HW]; ur[c] = gr[o + c * HW]; }
        const int xx = min(max(x + pad - col, 0), W - 1);
        float* __restrict__ out = dk + (((int64_t)b * H + y) * W + x) * 2 * kk;
        for (int i0 = 0; i0 < ks; i0 += rows_per_iter) {
            const int fi = i0 + row;
            if (lane_on && fi < ks) {
                const int yy = min(max(y + pad - fi, 0), H - 1);
                const float* px = img_b + ((int64_t)yy * W + xx);
                float sl = 0.0f, sr = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float v = px[c * HW];
                    sl += ul[c] * v;
                    sr += ur[c] * v;
                }
                __builtin_nontemporal_store(sl, out + fi * ks + col);
                __builtin_nontemporal_store(sr, out + kk + fi * ks + col);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// gradient with respect to the image
// ---------------------------------------------------------------------------
// Every kernel value is used once, on the C channels of one (unclamped) image position.  A workgroup owns a tile of
// kTile x kTile pixels and the (kTile + ks - 1)^2 positions their kernels reach -- the tile's halo, in padded
// coordinates -- and keeps the halo's sums in REGISTERS: thread t owns halo positions t, t + 256, ... (NACC of them,
// C sums each).  It streams the tile's kernels through LDS, `pix` consecutive pixels of a tile row at a time (one
// contiguous run of the PSF tensor, copied with 16-byte loads as the forward's k_local_psf_render_rows copies it:
// every PSF byte is read from HBM once, at full width), and after each copy every thread adds to its positions what
// those pixels' kernels send there: halo position (hv, hu) receives tap (yt + ks-1 - hv, xt + ks-1 - hu) of tile
// pixel (yt, xt).  Pixels are visited in a fixed order by the one thread that owns the sum: no atomics, the same
// bits every run.  The tile's halo goes to the workspace as partial[b][ty][tx][c][hv][hu]; k_render_grad_img_gather
// adds the overlapping halos and folds the padding into the border.
constexpr int kTile = 16;

__host__ __device__ inline int halo_side(int ks) { return kTile + ks - 1; }

// the staging of k_local_psf_render_rows (sdirt_render.hip): nfl floats from src to dst + sh, where sh = the run's
// misalignment in floats, so that source and destination stay congruent modulo 16 bytes
__device__ __forceinline__ float* stage_run(const float* __restrict__ src, int64_t first, int nfl, float* lds)
{
    typedef float fl4 __attribute__((ext_vector_type(4)));
    const int sh = (int)(first & 3);
    float* dst = lds + sh;
    const int head = min((4 - sh) & 3, nfl);
    const int nf4 = (nfl - head) >> 2;
    const fl4* src4 = reinterpret_cast<const fl4*>(src + head);
    fl4* dst4 = reinterpret_cast<fl4*>(dst + head);
    constexpr int STAGE_U = 8;
    for (int base = threadIdx.x; base < nf4; base += kBlock * STAGE_U) {
        fl4 v[STAGE_U];
#pragma unroll
        for (int u = 0; u < STAGE_U; ++u)
            if (base + u * kBlock < nf4) v[u] = __builtin_nontemporal_load(&src4[base + u * kBlock]);
#pragma unroll
        for (int u = 0; u < STAGE_U; ++u)
            if (base + u * kBlock < nf4) dst4[base + u * kBlock] = v[u];
    }
    if ((int)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (int i = head + (nf4 << 2) + threadIdx.x; i < nfl; i += kBlock) dst[i] = src[i];
    return dst;
}

template <int C, int NACC>
__global__ void __launch_bounds__(kBlock)
k_render_grad_img_tiles(const float* __restrict__ psf, const float* __restrict__ gl, const float* __restrict__ gr,
                        int H, int W, int ks, int pix, float* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float wts[];     // 4 + [pix][2][ks*ks]
    const int kk = ks * ks, side = halo_side(ks), npos = side * side;
    const int b = blockIdx.z, y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    const int64_t HW = (int64_t)H * W;
    // this thread's halo positions: row hv[k], and the LDS index of tap (ks-1 - hv, ks-1 - hu) of a kernel
    int hv[NACC], hu[NACC];
    float acc[NACC][C];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const int p = threadIdx.x + k * kBlock;
        hv[k] = p < npos ? p / side : (1 << 20);                    // a position past the halo matches no tap
        hu[k] = p - (p / side) * side;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[k][c] = 0.0f;
    }
    const int rows = min(kTile, H - y0), cols = min(kTile, W - x0);
    for (int yt = 0; yt < rows; ++yt) {
        for (int xs = 0; xs < cols; xs += pix) {
            const int np = min(pix, cols - xs);
            const int64_t pixel = ((int64_t)b * H + y0 + yt) * W + x0 + xs;
            const float* kl = stage_run(psf + pixel * 2 * kk, pixel * 2 * kk, np * 2 * kk, wts);
            __syncthreads();
            for (int q = 0; q < np; ++q) {
                const int64_t o = (int64_t)b * C * HW + (int64_t)(y0 + yt) * W + x0 + xs + q;     // block-uniform
                float ul[C], ur[C];
#pragma unroll
                for (int c = 0; c < C; ++c) { ul[c] = gl[o + c * HW]; ur[c] = gr[o + c * HW]; }
                const float* kq = kl + q * 2 * kk;
#pragma unroll
                for (int k = 0; k < NACC; ++k) {
                    const int i = yt + ks - 1 - hv[k], j = xs + q + ks - 1 - hu[k];
                    if ((unsigned)i < (unsigned)ks && (unsigned)j < (unsigned)ks) {
                        const float wl = kq[i * ks + j], wr = kq[kk + i * ks + j];
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[k][c] += ul[c] * wl + ur[c] * wr;
                    }
                }
            }
            __syncthreads();
        }
    }
    const int64_t tile = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    float* __restrict__ out = partial + tile * C * npos;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const int p = threadIdx.x + k * kBlock;
        if (p < npos) {
#pragma unroll
            for (int c = 0; c < C; ++c) out[(int64_t)c * npos + p] = acc[k][c];
        }
    }
}

// dImg[b,c,v,u] = the sum of every tile's halo value at the padded positions (v', u') that clamp to (v, u): v' = v
// inside the image, -pad..0 on the first row, H-1..H-1+pad on the last (both on an image of one row); the tiles
// that hold v' are those with ty * kTile - pad <= v' <= ty * kTile + kTile-1 + pad.  One thread per image value,
// a fixed order.
__global__ void __launch_bounds__(kBlock)
k_render_grad_img_gather(const float* __restrict__ partial, int B, int C, int H, int W, int ks,
                         float* __restrict__ dimg)
{
    const int pad = (ks - 1) / 2, side = halo_side(ks), npos = side * side;
    const int nty = (H + kTile - 1) / kTile, ntx = (W + kTile - 1) / kTile;
    const int64_t total = (int64_t)B * C * H * W;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int u = (int)(e % W), v = (int)((e / W) % H);
        const int c = (int)((e / ((int64_t)H * W)) % C), b = (int)(e / ((int64_t)C * H * W));
        const int v_lo = v == 0 ? -pad : v, v_hi = v == H - 1 ? H - 1 + pad : v;
        const int u_lo = u == 0 ? -pad : u, u_hi = u == W - 1 ? W - 1 + pad : u;
        float sum = 0.0f;
        for (int vp = v_lo; vp <= v_hi; ++vp) {
            // floor((vp + pad) / kTile) and ceil((vp - pad - (kTile - 1)) / kTile) = floor((vp - pad) / kTile)
            const int ty_hi = min((vp + pad) / kTile, nty - 1), ty_lo = max(vp - pad, 0) / kTile;
            for (int up = u_lo; up <= u_hi; ++up) {
                const int tx_hi = min((up + pad) / kTile, ntx - 1), tx_lo = max(up - pad, 0) / kTile;
                for (int ty = ty_lo; ty <= ty_hi; ++ty)
                    for (int tx = tx_lo; tx <= tx_hi; ++tx) {
                        const int64_t tile = ((int64_t)b * nty + ty) * ntx + tx;
                        const int p = (vp - ty * kTile + pad) * side + (up - tx * kTile + pad);
                        sum += partial[(tile * C + c) * npos + p];
                    }
            }
        }
        dimg[e] = sum;
    }
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
namespace {

// the argument rules of sdirt_local_psf_render (check_image_call) with the limits of these kernels' launch geometry:
// ks <= 64 (a kernel row per 64 lanes, the tile's kernels in 64 KB of LDS), B and H in a grid dimension
constexpr int kMaxKsGrad = 64;

dim3 tile_grid(int B, int H, int W)
{
    return dim3((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile), (unsigned)B);
}

template <int C, int NACC>
int launch_img_tiles(const float* psf, const float* gl, const float* gr, int B, int H, int W, int ks, float* partial,
                     hipStream_t st)
{
    const size_t per_pixel = sizeof(float) * 2 * (size_t)ks * ks;
    const int pix = per_pixel * 8 + 16 <= 64 * 1024 ? 8 : per_pixel * 4 + 16 <= 64 * 1024 ? 4 : 2;
    const size_t lds = per_pixel * pix + 16;
    if (lds > 48 * 1024)
        if (int rc = allow_large_lds<&k_render_grad_img_tiles<C, NACC>>(64 * 1024)) return rc;
    k_render_grad_img_tiles<C, NACC><<<tile_grid(B, H, W), kBlock, lds, st>>>(psf, gl, gr, H, W, ks, pix, partial);
    return SDIRT_OK;
}

// halo positions per thread: 6 up to ks 21 (36^2 / 256), 9 up to ks 33, 24 up to ks 63 (78^2 / 256)
template <int C>
int launch_img(const float* psf, const float* gl, const float* gr, int B, int H, int W, int ks, float* partial,
               hipStream_t st)
{
    const int nacc = (halo_side(ks) * halo_side(ks) + kBlock - 1) / kBlock;
    if (nacc <= 6) return launch_img_tiles<C, 6>(psf, gl, gr, B, H, W, ks, partial, st);
    if (nacc <= 9) return launch_img_tiles<C, 9>(psf, gl, gr, B, H, W, ks, partial, st);
    return launch_img_tiles<C, 24>(psf, gl, gr, B, H, W, ks, partial, st);
}

}  // namespace

extern "C" {

int sdirt_local_psf_render_grad_psf(const float* img, const float* grad_l, const float* grad_r, int32_t B, int32_t C,
                                    int32_t H, int32_t W, int32_t ks, float* grad_psf, void* stream)
{
    if (int rc = check_image_call({img, grad_l, grad_r, grad_psf}, B, C, H, W, ks, kMaxKsGrad, true)) return rc;
    if (B == 0) return SDIRT_OK;
    const dim3 grid((unsigned)((W + kGradChunk - 1) / kGradChunk), (unsigned)H, (unsigned)B);
    hipStream_t st = as_stream(stream);
    with_channels(C, [&](auto c) {                                    // C is one of them: checked above
        k_render_grad_psf<decltype(c)::value><<<grid, kBlock, 0, st>>>(img, grad_l, grad_r, H, W, ks, grad_psf);
        return SDIRT_OK;
    });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int64_t sdirt_local_psf_render_grad_img_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t ks)
{
    if (B < 0 || C < 1 || H < 1 || W < 1 || ks < 1 || ks > kMaxKsGrad || (ks & 1) == 0) return -1;
    const dim3 g = tile_grid(B, H, W);
    return (int64_t)sizeof(float) * B * g.y * g.x * C * halo_side(ks) * halo_side(ks);
}

int sdirt_local_psf_render_grad_img(const float* psf, const float* grad_l, const float* grad_r, int32_t B, int32_t C,
                                    int32_t H, int32_t W, int32_t ks, float* grad_img, void* workspace,
                                    int64_t workspace_bytes, void* stream)
{
    if (int rc = check_image_call({psf, grad_l, grad_r, grad_img}, B, C, H, W, ks, kMaxKsGrad, true)) return rc;
    if (B == 0) return SDIRT_OK;
    const int64_t need = sdirt_local_psf_render_grad_img_workspace_bytes(B, C, H, W, ks);
    if (!workspace || workspace_bytes < need)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)need);
    hipStream_t st = as_stream(stream);
    float* partial = static_cast<float*>(workspace);
    const int rc = with_channels(C, [&](auto c) {
        return launch_img<decltype(c)::value>(psf, grad_l, grad_r, B, H, W, ks, partial, st);
    });
    if (rc) return rc;
    LAUNCH_CHECK();
    const int grid = grid_for((int64_t)B * C * H * W, kBlock, 256 * 32);
    k_render_grad_img_gather<<<grid, kBlock, 0, st>>>(partial, B, C, H, W, ks, grad_img);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

}  // extern "C"
