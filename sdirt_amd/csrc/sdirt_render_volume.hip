// sdirt_render_volume.hip -- an RGB-D frame rendered into a dual-pixel pair straight from a ray-traced PSF volume
// (MI355X / gfx950 only), and the gradients of that render with respect to the volume, the image and the depth table
// value fz.
//
// V [Dz,Gy,Gx,2,ks,ks] holds one L/R kernel pair per grid node.  The kernel of a pixel is the trilinear interpolation
// of the eight nodes around it, K = sum_corners w * V[corner], w = (wz * wy) * wx with each factor f or 1 - f of the
// segment tables (per column ix, fx; per row iy, fy; per pixel iz, fz), and the convolution is the one of
// sdirt_local_psf_render (deeplens/render_psf.py:157-188: replicate padding, flipped taps):
//   out_s[b,c,y,x]       = sum_{i,j} K[s,i,j] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)],       pad = (ks - 1) / 2
//   dV[dz,gy,gx,s,i,j]   = sum_{b,y,x} w(y,x; node) * sum_c G_s[b,c,y,x] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)]
// The per-pixel kernels exist in registers only.  fp32 operands and sums, no atomics: every sum is taken by one
// thread (or one wave's butterfly) in a fixed order.  The tables are operands: an index outside [0, n-2] is clamped,
// the upper node of a segment is min(i + 1, n - 1), so no table value can make a kernel read outside V.
//
// A CHROMATIC volume [C,Dz,Gy,Gx,2,ks,ks] holds one such V per image channel (the three wavelengths of psf_rgb,
// deeplens/optics.py:999-1015): channel c is rendered with V[c], which lies c * Dz*Gy*Gx*2*ks*ks floats after V[0].
// The k_*_chroma kernels are siblings of the four achromatic ones: same geometry, same helpers in the same order, so
// one channel of a chromatic call has the bits of the achromatic call at C = 1 on that channel's slices.  Forward and
// depth gradient form a pixel's corners once for all channels; the other two take the channel as a grid dimension.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/sdirt_dp.h"
#include "sdirt_device.hpp"
#include "sdirt_host.hpp"
#include "sdirt_render.hpp"

using namespace sdirt;

namespace {

constexpr int kMaxKsVolume = 63;
constexpr int kPixChunk = 16;              // pixels of a row per workgroup of the forward (4 per wave)

// The six segment tables, which every kernel reads and none writes: one kernel parameter, by value.  (The six
// extents stay plain int parameters: as members of a by-value struct they change the forward's register allocation
// -- 35 VGPRs for 66 at C = 3, the sixteen corner loads of a tap no longer in flight together.)
struct SegmentTables {
    const int* ix; const float* fx;        // [W]
    const int* iy; const float* fy;        // [H]
    const int* iz; const float* fz;        // [B,H,W]
};

// The segment (i, f) of a table on an axis of n nodes: its two nodes, whatever the table holds -- the lower clamped
// to [0, n - 2], the upper min(lo + 1, n - 1), the lower again on an axis of one node -- and their weights 1 - f, f.
struct Segment {
    int lo, hi;
    float w_lo, w_hi;
    __device__ __forceinline__ Segment(int i, float f, int n)
        : lo(min(max(i, 0), max(n - 2, 0))), hi(min(lo + 1, n - 1)), w_lo(1.0f - f), w_hi(f) {}
    // g is one of the segment's two nodes
    __device__ __forceinline__ bool touches(int g) const { return lo == g || hi == g; }
};

// The weight of node g in the segment: 1 - f as the lower node, f as the upper; both on an axis of one node.
__device__ __forceinline__ float node_weight(const Segment& s, int g)
{
    const float a = s.lo == g ? s.w_lo : 0.0f, b = s.hi == g ? s.w_hi : 0.0f;
    return s.lo == s.hi ? a + b : (s.lo == g ? a : b);
}

// The eight nodes around a pixel, corner k = 4 * (z upper) + 2 * (y upper) + (x upper): the L kernel of each (its R
// kernel follows kk = ks*ks floats on) and its weight (wz * wy) * wx -- or, d_fz, the weight's derivative in fz,
// +-(wy * wx): + for the upper depth plane, - for the lower, each product formed once and used with both signs.
struct Corners {
    float w[8];
    const float* v[8];
    __device__ __forceinline__ Corners(const float* vol, int Gy, int Gx, int kk, const Segment& z, const Segment& y,
                                       const Segment& x, bool d_fz = false)
    {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int zz = k & 4 ? z.hi : z.lo, yy = k & 2 ? y.hi : y.lo, xx = k & 1 ? x.hi : x.lo;
            w[k] = ((k & 4 ? z.w_hi : z.w_lo) * (k & 2 ? y.w_hi : y.w_lo)) * (k & 1 ? x.w_hi : x.w_lo);
            v[k] = vol + (((int64_t)zz * Gy + yy) * Gx + xx) * 2 * kk;
        }
        if (d_fz) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float wyx = (k & 2 ? y.w_hi : y.w_lo) * (k & 1 ? x.w_hi : x.w_lo);
                w[k] = -wyx;
                w[k + 4] = wyx;
            }
        }
    }
};

// tap t of the interpolated L and R kernels, the corners added in order
__device__ __forceinline__ void kernel_tap(const Corners& cn, int t, int kk, float& kl, float& kr)
{
    kl = 0.0f;
    kr = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        kl += cn.w[k] * cn.v[k][t];
        kr += cn.w[k] * cn.v[k][kk + t];
    }
}

// Tap t of channel c of a chromatic volume, whose channels lie ch floats apart, as the tap index kernel_tap takes.
// The sum is made opaque and kept in a VGPR: left to the compiler, the wave-uniform c * ch is folded into the corner
// pointers, C sets of eight -- in the forward they no longer fit the SGPRs (73 v_writelane spills and a wait after
// every load at C = 3).
__device__ __forceinline__ int channel_tap(int c, int ch, int t)
{
    int tc = c * ch + t;
    asm("" : "+v"(tc));
    return tc;
}

// Tap t of the interpolated L and R kernels of all C channels, the 16 C corner values read before the first of them is
// used: per channel kernel_tap's sums in kernel_tap's order.
template <int C>
__device__ __forceinline__ void kernel_taps(const Corners& cn, int ch, int t, int kk, float (&kl)[C], float (&kr)[C])
{
    float vl[C][8], vr[C][8];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int tc = channel_tap(c, ch, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            vl[c][k] = cn.v[k][tc];
            vr[c][k] = cn.v[k][kk + tc];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        kl[c] = 0.0f;
        kr[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            kl[c] += cn.w[k] * vl[c][k];
            kr[c] += cn.w[k] * vr[c][k];
        }
    }
}

// Taps first, first + stride, ... of a ks x ks kernel as (row i, column j), without a division per step.  The two
// divisions are the constructor's: build the start state once, outside the loops, and copy it.
struct TapWalker {
    int i, j, di, dj, ks;
    __device__ __forceinline__ TapWalker(int first, int stride, int ks_)
        : i(first / ks_), j(first - i * ks_), di(stride / ks_), dj(stride - di * ks_), ks(ks_) {}
    __device__ __forceinline__ void next()
    {
        i += di;
        j += dj;
        if (j >= ks) { j -= ks; ++i; }
    }
};

// Channel 0 of the image at (yy, xx), clamped into the image (replicate padding).  Stored tap (i, j) of the kernel of
// pixel (y, x) multiplies the neighbour at the FLIPPED offset (render_psf.py:175): yy = y + pad - i, xx = x + pad - j.
__device__ __forceinline__ const float* clamped_pixel(const float* img_b, int yy, int xx, int H, int W)
{
    return img_b + ((int64_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1));
}

}  // namespace

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// One WAVE per output pixel, as k_local_psf_render: the lanes stride over the ks*ks taps; for its tap a lane reads the
// eight corner values of each side (consecutive lanes, consecutive addresses: 256-B segments of a volume that stays in
// L2 / Infinity Cache -- the pixels of a cell share their four (x, y) corners, and the workgroup's pixels are
// neighbours in a row), forms K_l, K_r and multiplies the C image values at the flipped, clamped offset.  The segment
// indices and weights are wave-uniform; the depth segment is read per pixel, nothing assumes a tile shares it.
template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume(const float* __restrict__ img, const float* __restrict__ vol, const SegmentTables tb, int H, int W,
                    int ks, int Dz, int Gy, int Gx, float* __restrict__ outl, float* __restrict__ outr)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.y, b = blockIdx.z, pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ img_b = img + (int64_t)b * C * HW;
    const TapWalker tap0(lane, 64, ks);
    const Segment sy(tb.iy[y], tb.fy[y], Gy);
    const int x_end = min(W, ((int)blockIdx.x + 1) * kPixChunk);
    for (int x = blockIdx.x * kPixChunk + wave; x < x_end; x += kBlock / 64) {
        const int64_t pixel = (int64_t)b * HW + (int64_t)y * W + x;
        const Corners cn(vol, Gy, Gx, kk, Segment(tb.iz[pixel], tb.fz[pixel], Dz), sy, Segment(tb.ix[x], tb.fx[x], Gx));
        float accl[C], accr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { accl[c] = 0.0f; accr[c] = 0.0f; }
        TapWalker tap = tap0;
        for (int t = lane; t < kk; t += 64) {
            float kl, kr;
            kernel_tap(cn, t, kk, kl, kr);
            const float* px = clamped_pixel(img_b, y + pad - tap.i, x + pad - tap.j, H, W);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float p = px[c * HW];
                accl[c] += kl * p;
                accr[c] += kr * p;
            }
            tap.next();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float a = accl[c], r = accr[c];
            shuffle_sum(a, r);
            if (lane == 0) {
                const int64_t o = ((int64_t)(b * C + c) * H + y) * W + x;
                outl[o] = a;
                outr[o] = r;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// gradient with respect to the volume
// ---------------------------------------------------------------------------
// One workgroup per ((x, y) node, side, chunk of depth planes).  Thread t owns taps t, t + 256, ... of every plane of
// the chunk; their sums live in LDS as acc[plane][tap] (each element is only ever touched by its owner, LDS is used
// for its dynamic indexing by plane, so the sums need no barrier and no atomic).  The workgroup first finds the
// columns and rows whose segment has this node as an end -- the smallest rectangle that holds them; with the monotone
// tables axis_segments makes that is the at most four cells around the node -- then walks the rectangle's pixels,
// batch by batch, image by image, in raster order.  A batch of 256 pixels is prepared by the 256 threads (weights,
// planes, the C upstream values of this side) and left in LDS; then every thread adds, pixel after pixel,
//   D = sum_c G[c] * img[c, clamp(y+pad-i), clamp(x+pad-j)]        acc[plane0][tap] += w0 * D, acc[plane1][tap] += w1 * D
// for its taps.  Pixels whose weight at the node is 0, or whose planes lie in another chunk, are skipped.  At the end
// the chunk's block of dV is written, every element once: nodes no pixel touches get the zeros acc started with.
template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_grad(const float* __restrict__ img, const float* __restrict__ gl, const float* __restrict__ gr,
                         const SegmentTables tb, int B, int H, int W, int ks, int Dz, int Gy, int Gx, int planes,
                         float* __restrict__ dvol)
{
    extern __shared__ __attribute__((aligned(16))) float acc[];          // [planes][ks*ks]
    __shared__ float s_w0[kBlock], s_w1[kBlock], s_g[C][kBlock];
    __shared__ int s_l0[kBlock], s_l1[kBlock], s_y[kBlock], s_x[kBlock];
    __shared__ int s_range[4][kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gx = blockIdx.x % Gx, gy = blockIdx.x / Gx, side = blockIdx.y;
    const int z_first = blockIdx.z * planes, nz = min(planes, Dz - z_first);
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ gs = side ? gr : gl;
    const TapWalker tap0(tid, kBlock, ks);

    for (int l = 0; l < nz; ++l)
        for (int t = tid; t < kk; t += kBlock) acc[l * kk + t] = 0.0f;

    // the columns [x_lo, x_hi) and rows [y_lo, y_hi) that hold every pixel touching this node
    int x_lo = W, x_hi = 0, y_lo = H, y_hi = 0;
    for (int x = tid; x < W; x += kBlock)
        if (Segment(tb.ix[x], 0.0f, Gx).touches(gx)) { x_lo = min(x_lo, x); x_hi = max(x_hi, x + 1); }
    for (int y = tid; y < H; y += kBlock)
        if (Segment(tb.iy[y], 0.0f, Gy).touches(gy)) { y_lo = min(y_lo, y); y_hi = max(y_hi, y + 1); }
    for (int off = 32; off > 0; off >>= 1) {
        x_lo = min(x_lo, __shfl_xor(x_lo, off));
        x_hi = max(x_hi, __shfl_xor(x_hi, off));
        y_lo = min(y_lo, __shfl_xor(y_lo, off));
        y_hi = max(y_hi, __shfl_xor(y_hi, off));
    }
    if (lane == 0) { s_range[0][wave] = x_lo; s_range[1][wave] = x_hi; s_range[2][wave] = y_lo; s_range[3][wave] = y_hi; }
    __syncthreads();
    for (int k = 0; k < kBlock / 64; ++k) {
        x_lo = min(x_lo, s_range[0][k]);
        x_hi = max(x_hi, s_range[1][k]);
        y_lo = min(y_lo, s_range[2][k]);
        y_hi = max(y_hi, s_range[3][k]);
    }
    const int nx = max(x_hi - x_lo, 0), ny = max(y_hi - y_lo, 0);
    const int64_t npix = (int64_t)nx * ny;

    for (int b = 0; b < B; ++b) {
        const float* __restrict__ img_b = img + (int64_t)b * C * HW;
        for (int64_t first = 0; first < npix; first += kBlock) {
            __syncthreads();                                             // the previous batch has been consumed
            const int64_t p = first + tid;
            int l0 = -1, l1 = -1;
            if (p < npix) {
                const int y = y_lo + (int)(p / nx), x = x_lo + (int)(p - (p / nx) * nx);
                const Segment sy(tb.iy[y], tb.fy[y], Gy), sx(tb.ix[x], tb.fx[x], Gx);
                const bool touches = sy.touches(gy) && sx.touches(gx);
                const float wy = node_weight(sy, gy), wx = node_weight(sx, gx);
                const int64_t pixel = (int64_t)b * HW + (int64_t)y * W + x;
                const Segment sz(tb.iz[pixel], tb.fz[pixel], Dz);
                const float w0 = (sz.w_lo * wy) * wx, w1 = (sz.w_hi * wy) * wx;
                if (touches && w0 != 0.0f && sz.lo >= z_first && sz.lo < z_first + nz) l0 = sz.lo - z_first;
                if (touches && w1 != 0.0f && sz.hi >= z_first && sz.hi < z_first + nz) l1 = sz.hi - z_first;
                s_w0[tid] = w0;
                s_w1[tid] = w1;
                s_y[tid] = y + pad;
                s_x[tid] = x + pad;
#pragma unroll
                for (int c = 0; c < C; ++c) s_g[c][tid] = gs[(int64_t)b * C * HW + c * HW + (int64_t)y * W + x];
            }
            s_l0[tid] = l0;
            s_l1[tid] = l1;
            __syncthreads();
            const int n = (int)min((int64_t)kBlock, npix - first);
            for (int q = 0; q < n; ++q) {
                const int q0 = __builtin_amdgcn_readfirstlane(s_l0[q]), q1 = __builtin_amdgcn_readfirstlane(s_l1[q]);
                if (q0 < 0 && q1 < 0) continue;
                const float w0 = s_w0[q], w1 = s_w1[q];
                const int yb = s_y[q], xb = s_x[q];
                float u[C];
#pragma unroll
                for (int c = 0; c < C; ++c) u[c] = s_g[c][q];
                TapWalker tap = tap0;
                for (int t = tid; t < kk; t += kBlock) {
                    const float* px = clamped_pixel(img_b, yb - tap.i, xb - tap.j, H, W);
                    float d = u[0] * px[0];
#pragma unroll
                    for (int c = 1; c < C; ++c) d += u[c] * px[c * HW];
                    if (q0 >= 0) acc[q0 * kk + t] += w0 * d;
                    if (q1 >= 0) acc[q1 * kk + t] += w1 * d;
                    tap.next();
                }
            }
        }
    }
    for (int l = 0; l < nz; ++l) {
        float* __restrict__ out = dvol + ((((int64_t)(z_first + l) * Gy + gy) * Gx + gx) * 2 + side) * kk;
        for (int t = tid; t < kk; t += kBlock) out[t] = acc[l * kk + t];
    }
}

// ---------------------------------------------------------------------------
// gradients with respect to the scene: the depth table value fz and the image
// ---------------------------------------------------------------------------
// dfz[b,y,x] = sum_s sum_c G_s[b,c,y,x] * sum_{i,j} (dK_s/dfz)[i,j] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)], where
// dK_s/dfz = sum_corners +-(wy * wx) * V[corner]: + for the upper depth plane, - for the lower (K is linear in fz, so
// fz itself is not an operand).  The forward's geometry: one wave per pixel, the lanes stride over the taps, the
// corner pointers and weights are wave-uniform.  Per tap the 2C upstream values are folded into
// D_s = sum_c G_s[c] * img[c, .] first; a butterfly sums the lanes, one store per pixel.  A pixel whose two depth
// planes are the same node (an axis of one node) gets exactly 0, not the rounded difference of equal sums.
template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_grad_depth(const float* __restrict__ img, const float* __restrict__ vol,
                               const float* __restrict__ gl, const float* __restrict__ gr, const SegmentTables tb,
                               int H, int W, int ks, int Dz, int Gy, int Gx, float* __restrict__ dfz)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.y, b = blockIdx.z, pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ img_b = img + (int64_t)b * C * HW;
    const TapWalker tap0(lane, 64, ks);
    const Segment sy(tb.iy[y], tb.fy[y], Gy);
    const int x_end = min(W, ((int)blockIdx.x + 1) * kPixChunk);
    for (int x = blockIdx.x * kPixChunk + wave; x < x_end; x += kBlock / 64) {
        const int64_t pixel = (int64_t)b * HW + (int64_t)y * W + x;
        const Segment sz(tb.iz[pixel], 0.0f, Dz);                        // K is linear in fz: its value is no operand
        float acc = 0.0f;
        if (sz.lo != sz.hi) {
            const Corners cn(vol, Gy, Gx, kk, sz, sy, Segment(tb.ix[x], tb.fx[x], Gx), true);
            float ul[C], ur[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int64_t o = (int64_t)b * C * HW + c * HW + (int64_t)y * W + x;
                ul[c] = gl[o];
                ur[c] = gr[o];
            }
            TapWalker tap = tap0;
            for (int t = lane; t < kk; t += 64) {
                float kl, kr;
                kernel_tap(cn, t, kk, kl, kr);
                const float* px = clamped_pixel(img_b, y + pad - tap.i, x + pad - tap.j, H, W);
                float dl = 0.0f, dr = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float p = px[c * HW];
                    dl += ul[c] * p;
                    dr += ur[c] * p;
                }
                acc += kl * dl + kr * dr;
                tap.next();
            }
            acc = shuffle_sum(acc);
        }
        if (lane == 0) dfz[pixel] = acc;
    }
}

// dImg[b,c,v,u] = sum_s sum_{(y,x,i,j): clamp(y+pad-i) = v, clamp(x+pad-j) = u} G_s[b,c,y,x] * K_s(b,y,x)[i,j]: a gather,
// one wave per image position (v, u), all C channels.  The lanes stride over the ks*ks output pixels
// (y, x) = (v - pad + yr, u - pad + xr) whose kernels reach the position; those outside the image have no term.  Inside
// the image pixel (y, x) reaches (v, u) with the one tap (i, j) = (yr, xr) -- consecutive lanes are consecutive pixels
// and consecutive taps, so with a smooth depth they read consecutive addresses of the same corners.  On a border the
// position also collects every padded position that clamps onto it (k_render_grad_img_gather, sdirt_render_grad.hip):
// on the first row the taps i >= yr, on the last the taps i <= yr, on an image of one row all of them; columns
// likewise.  The upstream values do not depend on the tap, so a lane first sums its pixel's kernel over the tap
// range, S_s = sum_{i,j} K_s[i,j], then adds G_l[c] * S_l + G_r[c] * S_r.  Unlike the forward, the segment, the eight
// weights and the corner offsets vary per lane.  Fixed order throughout, a butterfly at the end, one store per channel.
template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_grad_img(const float* __restrict__ vol, const float* __restrict__ gl, const float* __restrict__ gr,
                             const SegmentTables tb, int H, int W, int ks, int Dz, int Gy, int Gx,
                             float* __restrict__ dimg)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int v = blockIdx.y, b = blockIdx.z;
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ gl_b = gl + (int64_t)b * C * HW;
    const float* __restrict__ gr_b = gr + (int64_t)b * C * HW;
    const TapWalker rel0(lane, 64, ks);                                 // (yr, xr) = (rel.i, rel.j)
    const int u_end = min(W, ((int)blockIdx.x + 1) * kPixChunk);
    for (int u = blockIdx.x * kPixChunk + wave; u < u_end; u += kBlock / 64) {
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;
        TapWalker rel = rel0;
        for (int p = lane; p < kk; p += 64) {
            const int y = v - pad + rel.i, x = u - pad + rel.j;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                // the taps of pixel (y, x) that read a padded position clamping onto (v, u)
                const int i_lo = v == H - 1 ? 0 : rel.i, i_hi = v == 0 ? ks - 1 : rel.i;
                const int j_lo = u == W - 1 ? 0 : rel.j, j_hi = u == 0 ? ks - 1 : rel.j;
                const int64_t pixel = (int64_t)y * W + x;
                const Corners cn(vol, Gy, Gx, kk,
                                 Segment(tb.iz[(int64_t)b * HW + pixel], tb.fz[(int64_t)b * HW + pixel], Dz),
                                 Segment(tb.iy[y], tb.fy[y], Gy), Segment(tb.ix[x], tb.fx[x], Gx));
                float sl = 0.0f, sr = 0.0f;
                for (int i = i_lo; i <= i_hi; ++i)
                    for (int j = j_lo; j <= j_hi; ++j) {
                        float kl, kr;
                        kernel_tap(cn, i * ks + j, kk, kl, kr);
                        sl += kl;
                        sr += kr;
                    }
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += gl_b[c * HW + pixel] * sl + gr_b[c * HW + pixel] * sr;
            }
            rel.next();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float a = shuffle_sum(acc[c]);
            if (lane == 0) dimg[((int64_t)(b * C + c) * H + v) * W + u] = a;
        }
    }
}

// ---------------------------------------------------------------------------
// chromatic volumes: one V per channel
// ---------------------------------------------------------------------------
// The forward of a chromatic volume: k_render_psf_volume with K_l[c], K_r[c] per channel -- 16 C corner values per tap,
// the corners of a channel added in kernel_tap's order, one pixel value per channel.
template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_chroma(const float* __restrict__ img, const float* __restrict__ vol, const SegmentTables tb, int H,
                           int W, int ks, int Dz, int Gy, int Gx, float* __restrict__ outl, float* __restrict__ outr)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.y, b = blockIdx.z, pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const int ch = Dz * Gy * Gx * 2 * kk;                              // floats of one channel's V (the entry checks C * ch)
    const float* __restrict__ img_b = img + (int64_t)b * C * HW;
    const TapWalker tap0(lane, 64, ks);
    const Segment sy(tb.iy[y], tb.fy[y], Gy);
    const int x_end = min(W, ((int)blockIdx.x + 1) * kPixChunk);
    for (int x = blockIdx.x * kPixChunk + wave; x < x_end; x += kBlock / 64) {
        const int64_t pixel = (int64_t)b * HW + (int64_t)y * W + x;
        const Corners cn(vol, Gy, Gx, kk, Segment(tb.iz[pixel], tb.fz[pixel], Dz), sy, Segment(tb.ix[x], tb.fx[x], Gx));
        float accl[C], accr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { accl[c] = 0.0f; accr[c] = 0.0f; }
        TapWalker tap = tap0;
        for (int t = lane; t < kk; t += 64) {
            const float* px = clamped_pixel(img_b, y + pad - tap.i, x + pad - tap.j, H, W);
            float kl[C], kr[C];
            kernel_taps<C>(cn, ch, t, kk, kl, kr);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float p = px[c * HW];
                accl[c] += kl[c] * p;
                accr[c] += kr[c] * p;
            }
            tap.next();
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float a = accl[c], r = accr[c];
            shuffle_sum(a, r);
            if (lane == 0) {
                const int64_t o = ((int64_t)(b * C + c) * H + y) * W + x;
                outl[o] = a;
                outr[o] = r;
            }
        }
    }
}

// dV[c,dz,gy,gx,s,i,j] = sum_{b,y,x} w(y,x; node) * G_s[b,c,y,x] * img[b,c,clamp(y+pad-i),clamp(x+pad-j)]: no sum over
// the channels.  k_render_psf_volume_grad<1> on channel c of C, the channel a grid dimension: one workgroup per
// ((x, y) node, (channel, side), chunk of depth planes), blockIdx.y = 2 c + side; the LDS budget and the chunks are
// those of one channel.  Every element of dV is written once, by the workgroup of its channel.
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_chroma_grad(const float* __restrict__ img, const float* __restrict__ gl,
                                const float* __restrict__ gr, const SegmentTables tb, int B, int C, int H, int W, int ks,
                                int Dz, int Gy, int Gx, int planes, float* __restrict__ dvol)
{
    extern __shared__ __attribute__((aligned(16))) float acc[];          // [planes][ks*ks]
    __shared__ float s_w0[kBlock], s_w1[kBlock], s_g[kBlock];
    __shared__ int s_l0[kBlock], s_l1[kBlock], s_y[kBlock], s_x[kBlock];
    __shared__ int s_range[4][kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gx = blockIdx.x % Gx, gy = blockIdx.x / Gx, side = blockIdx.y & 1, c = blockIdx.y >> 1;
    const int z_first = blockIdx.z * planes, nz = min(planes, Dz - z_first);
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ gs = (side ? gr : gl) + c * HW;
    const TapWalker tap0(tid, kBlock, ks);

    for (int l = 0; l < nz; ++l)
        for (int t = tid; t < kk; t += kBlock) acc[l * kk + t] = 0.0f;

    // the columns [x_lo, x_hi) and rows [y_lo, y_hi) that hold every pixel touching this node
    int x_lo = W, x_hi = 0, y_lo = H, y_hi = 0;
    for (int x = tid; x < W; x += kBlock)
        if (Segment(tb.ix[x], 0.0f, Gx).touches(gx)) { x_lo = min(x_lo, x); x_hi = max(x_hi, x + 1); }
    for (int y = tid; y < H; y += kBlock)
        if (Segment(tb.iy[y], 0.0f, Gy).touches(gy)) { y_lo = min(y_lo, y); y_hi = max(y_hi, y + 1); }
    for (int off = 32; off > 0; off >>= 1) {
        x_lo = min(x_lo, __shfl_xor(x_lo, off));
        x_hi = max(x_hi, __shfl_xor(x_hi, off));
        y_lo = min(y_lo, __shfl_xor(y_lo, off));
        y_hi = max(y_hi, __shfl_xor(y_hi, off));
    }
    if (lane == 0) { s_range[0][wave] = x_lo; s_range[1][wave] = x_hi; s_range[2][wave] = y_lo; s_range[3][wave] = y_hi; }
    __syncthreads();
    for (int k = 0; k < kBlock / 64; ++k) {
        x_lo = min(x_lo, s_range[0][k]);
        x_hi = max(x_hi, s_range[1][k]);
        y_lo = min(y_lo, s_range[2][k]);
        y_hi = max(y_hi, s_range[3][k]);
    }
    const int nx = max(x_hi - x_lo, 0), ny = max(y_hi - y_lo, 0);
    const int64_t npix = (int64_t)nx * ny;

    for (int b = 0; b < B; ++b) {
        const float* __restrict__ img_c = img + ((int64_t)b * C + c) * HW;
        for (int64_t first = 0; first < npix; first += kBlock) {
            __syncthreads();                                             // the previous batch has been consumed
            const int64_t p = first + tid;
            int l0 = -1, l1 = -1;
            if (p < npix) {
                const int y = y_lo + (int)(p / nx), x = x_lo + (int)(p - (p / nx) * nx);
                const Segment sy(tb.iy[y], tb.fy[y], Gy), sx(tb.ix[x], tb.fx[x], Gx);
                const bool touches = sy.touches(gy) && sx.touches(gx);
                const float wy = node_weight(sy, gy), wx = node_weight(sx, gx);
                const int64_t pixel = (int64_t)b * HW + (int64_t)y * W + x;
                const Segment sz(tb.iz[pixel], tb.fz[pixel], Dz);
                const float w0 = (sz.w_lo * wy) * wx, w1 = (sz.w_hi * wy) * wx;
                if (touches && w0 != 0.0f && sz.lo >= z_first && sz.lo < z_first + nz) l0 = sz.lo - z_first;
                if (touches && w1 != 0.0f && sz.hi >= z_first && sz.hi < z_first + nz) l1 = sz.hi - z_first;
                s_w0[tid] = w0;
                s_w1[tid] = w1;
                s_y[tid] = y + pad;
                s_x[tid] = x + pad;
                s_g[tid] = gs[(int64_t)b * C * HW + (int64_t)y * W + x];
            }
            s_l0[tid] = l0;
            s_l1[tid] = l1;
            __syncthreads();
            const int n = (int)min((int64_t)kBlock, npix - first);
            for (int q = 0; q < n; ++q) {
                const int q0 = __builtin_amdgcn_readfirstlane(s_l0[q]), q1 = __builtin_amdgcn_readfirstlane(s_l1[q]);
                if (q0 < 0 && q1 < 0) continue;
                const float w0 = s_w0[q], w1 = s_w1[q], u = s_g[q];
                const int yb = s_y[q], xb = s_x[q];
                TapWalker tap = tap0;
                for (int t = tid; t < kk; t += kBlock) {
                    const float d = u * *clamped_pixel(img_c, yb - tap.i, xb - tap.j, H, W);
                    if (q0 >= 0) acc[q0 * kk + t] += w0 * d;
                    if (q1 >= 0) acc[q1 * kk + t] += w1 * d;
                    tap.next();
                }
            }
        }
    }
    for (int l = 0; l < nz; ++l) {
        float* __restrict__ out = dvol + (((((int64_t)c * Dz + z_first + l) * Gy + gy) * Gx + gx) * 2 + side) * kk;
        for (int t = tid; t < kk; t += kBlock) out[t] = acc[l * kk + t];
    }
}

// dfz of a chromatic volume: dK_s/dfz depends on the channel, so the upstream values cannot be folded before the
// kernel is applied as k_render_psf_volume_grad_depth does; per tap and channel
//   acc += G_l[c] * ((dK_l[c]/dfz) * img[c, .]) + G_r[c] * ((dK_r[c]/dfz) * img[c, .]).
// A pixel whose two depth planes are the same node gets exactly 0.
template <int C>
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_chroma_grad_depth(const float* __restrict__ img, const float* __restrict__ vol,
                                      const float* __restrict__ gl, const float* __restrict__ gr,
                                      const SegmentTables tb, int H, int W, int ks, int Dz, int Gy, int Gx,
                                      float* __restrict__ dfz)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.y, b = blockIdx.z, pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const int ch = Dz * Gy * Gx * 2 * kk;                              // floats of one channel's V (the entry checks C * ch)
    const float* __restrict__ img_b = img + (int64_t)b * C * HW;
    const TapWalker tap0(lane, 64, ks);
    const Segment sy(tb.iy[y], tb.fy[y], Gy);
    const int x_end = min(W, ((int)blockIdx.x + 1) * kPixChunk);
    for (int x = blockIdx.x * kPixChunk + wave; x < x_end; x += kBlock / 64) {
        const int64_t pixel = (int64_t)b * HW + (int64_t)y * W + x;
        const Segment sz(tb.iz[pixel], 0.0f, Dz);                        // K is linear in fz: its value is no operand
        float acc = 0.0f;
        if (sz.lo != sz.hi) {
            const Corners cn(vol, Gy, Gx, kk, sz, sy, Segment(tb.ix[x], tb.fx[x], Gx), true);
            float ul[C], ur[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int64_t o = (int64_t)b * C * HW + c * HW + (int64_t)y * W + x;
                ul[c] = gl[o];
                ur[c] = gr[o];
            }
            TapWalker tap = tap0;
            for (int t = lane; t < kk; t += 64) {
                const float* px = clamped_pixel(img_b, y + pad - tap.i, x + pad - tap.j, H, W);
                float kl[C], kr[C];
                kernel_taps<C>(cn, ch, t, kk, kl, kr);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float p = px[c * HW];
                    acc += ul[c] * (kl[c] * p) + ur[c] * (kr[c] * p);
                }
                tap.next();
            }
            acc = shuffle_sum(acc);
        }
        if (lane == 0) dfz[pixel] = acc;
    }
}

// dImg of a chromatic volume: k_render_psf_volume_grad_img<1> on channel c of C, the channel a grid dimension --
// blockIdx.x = c * chunks + (16 positions of a row), so that the workgroups in flight together work on one channel's
// volume, as three achromatic calls would.  (With the channels inside the wave, S_l[c], S_r[c] on shared per-lane
// corners, the scattered reads of the three volumes at once ran 1.7 times as long as those three calls.)
__global__ void __launch_bounds__(kBlock)
k_render_psf_volume_chroma_grad_img(const float* __restrict__ vol, const float* __restrict__ gl,
                                    const float* __restrict__ gr, const SegmentTables tb, int C, int H, int W, int ks,
                                    int Dz, int Gy, int Gx, int chunks, float* __restrict__ dimg)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
    const int v = blockIdx.y, b = blockIdx.z;
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t HW = (int64_t)H * W;
    const float* __restrict__ vol_c = vol + (int64_t)c * Dz * Gy * Gx * 2 * kk;
    const float* __restrict__ gl_c = gl + ((int64_t)b * C + c) * HW;
    const float* __restrict__ gr_c = gr + ((int64_t)b * C + c) * HW;
    const TapWalker rel0(lane, 64, ks);                                 // (yr, xr) = (rel.i, rel.j)
    const int u_end = min(W, (chunk + 1) * kPixChunk);
    for (int u = chunk * kPixChunk + wave; u < u_end; u += kBlock / 64) {
        float acc = 0.0f;
        TapWalker rel = rel0;
        for (int p = lane; p < kk; p += 64) {
            const int y = v - pad + rel.i, x = u - pad + rel.j;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                // the taps of pixel (y, x) that read a padded position clamping onto (v, u)
                const int i_lo = v == H - 1 ? 0 : rel.i, i_hi = v == 0 ? ks - 1 : rel.i;
                const int j_lo = u == W - 1 ? 0 : rel.j, j_hi = u == 0 ? ks - 1 : rel.j;
                const int64_t pixel = (int64_t)y * W + x;
                const Corners cn(vol_c, Gy, Gx, kk,
                                 Segment(tb.iz[(int64_t)b * HW + pixel], tb.fz[(int64_t)b * HW + pixel], Dz),
                                 Segment(tb.iy[y], tb.fy[y], Gy), Segment(tb.ix[x], tb.fx[x], Gx));
                float sl = 0.0f, sr = 0.0f;
                for (int i = i_lo; i <= i_hi; ++i)
                    for (int j = j_lo; j <= j_hi; ++j) {
                        float kl, kr;
                        kernel_tap(cn, i * ks + j, kk, kl, kr);
                        sl += kl;
                        sr += kr;
                    }
                acc += gl_c[pixel] * sl + gr_c[pixel] * sr;
            }
            rel.next();
        }
        acc = shuffle_sum(acc);
        if (lane == 0) dimg[(((int64_t)b * C + c) * H + v) * W + u] = acc;
    }
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
namespace {

// depth planes whose [ks*ks] sums fit in the 64 KiB of LDS a workgroup of the gradient asks for at most
constexpr int kGradLds = 64 * 1024;
int planes_per_chunk(int Dz, int ks) { return std::min(Dz, kGradLds / (int)(sizeof(float) * ks * ks)); }

// the shared shape rules, and the volume's own: every extent >= 1, a plane's nodes fit int32
int check_volume_render(const void* a, const void* b, const void* c, const void* d, const SegmentTables& tb, int B,
                        int C, int H, int W, int ks, int Dz, int Gy, int Gx)
{
    if (Dz < 1 || Gy < 1 || Gx < 1) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad shape (Dz, Gy, Gx must be >= 1)");
    if (int rc = check_image_call({a, b, c, d, tb.ix, tb.fx, tb.iy, tb.fy, tb.iz, tb.fz}, B, C, H, W, ks, kMaxKsVolume,
                                  true))
        return rc;
    if ((int64_t)Gy * Gx > INT32_MAX) return fail(SDIRT_ERR_UNSUPPORTED, "%d x %d nodes per plane", Gy, Gx);
    return SDIRT_OK;
}

// one wave per pixel (forward, depth gradient) or image position (image gradient)
dim3 pixel_grid(int B, int H, int W)
{
    return dim3((unsigned)((W + kPixChunk - 1) / kPixChunk), (unsigned)H, (unsigned)B);
}

template <int C>
int launch_volume_grad(dim3 grid, size_t lds, hipStream_t st, const float* img, const float* gl, const float* gr,
                       const SegmentTables& tb, int B, int H, int W, int ks, int Dz, int Gy, int Gx, int planes,
                       float* dvol)
{
    if (lds > 32 * 1024)
        if (int rc = allow_large_lds<&k_render_psf_volume_grad<C>>(kGradLds)) return rc;
    k_render_psf_volume_grad<C><<<grid, kBlock, lds, st>>>(img, gl, gr, tb, B, H, W, ks, Dz, Gy, Gx, planes, dvol);
    return SDIRT_OK;
}

// a chromatic volume's own rule: its kernels reach channel c by an int offset of the tap index
int check_chroma_volume(int C, int ks, int Dz, int Gy, int Gx)
{
    if ((int64_t)Dz * Gy * Gx > INT32_MAX / ((int64_t)2 * ks * ks * C))
        return fail(SDIRT_ERR_UNSUPPORTED, "a chromatic volume of %d x %d x %d x %d nodes at ks=%d (more than 2^31 - 1 floats)",
                    C, Dz, Gy, Gx, ks);
    return SDIRT_OK;
}

// The three entries, each for both kinds of volume: chroma = one V per channel, [C,Dz,Gy,Gx,2,ks,ks].

int render_volume(bool chroma, const float* img, const float* volume, const SegmentTables& tb, int B, int C, int H,
                  int W, int ks, int Dz, int Gy, int Gx, float* out_l, float* out_r, void* stream)
{
    if (int rc = check_volume_render(img, volume, out_l, out_r, tb, B, C, H, W, ks, Dz, Gy, Gx)) return rc;
    if (chroma)
        if (int rc = check_chroma_volume(C, ks, Dz, Gy, Gx)) return rc;
    if (B == 0) return SDIRT_OK;
    const dim3 grid = pixel_grid(B, H, W);
    hipStream_t st = as_stream(stream);
    with_channels(C, [&](auto c) {
        constexpr int Cc = decltype(c)::value;
        if (chroma)
            k_render_psf_volume_chroma<Cc><<<grid, kBlock, 0, st>>>(img, volume, tb, H, W, ks, Dz, Gy, Gx, out_l, out_r);
        else
            k_render_psf_volume<Cc><<<grid, kBlock, 0, st>>>(img, volume, tb, H, W, ks, Dz, Gy, Gx, out_l, out_r);
        return SDIRT_OK;
    });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int render_volume_grad(bool chroma, const float* img, const float* grad_l, const float* grad_r, const SegmentTables& tb,
                       int B, int C, int H, int W, int ks, int Dz, int Gy, int Gx, float* grad_volume, void* stream)
{
    if (int rc = check_volume_render(img, grad_l, grad_r, grad_volume, tb, B, C, H, W, ks, Dz, Gy, Gx)) return rc;
    if (chroma)
        if (int rc = check_chroma_volume(C, ks, Dz, Gy, Gx)) return rc;
    // (an empty batch is launched like any other: every element of grad_volume is written, all 0)
    const int planes = planes_per_chunk(Dz, ks), chunks = (Dz + planes - 1) / planes;
    if (chunks > 65535) return fail(SDIRT_ERR_UNSUPPORTED, "%d depth planes at ks=%d", Dz, ks);
    const size_t lds = sizeof(float) * (size_t)planes * ks * ks;
    hipStream_t st = as_stream(stream);
    if (chroma) {
        // the channel is a grid dimension: blockIdx.y = 2 c + side
        const dim3 grid((unsigned)(Gy * Gx), 2u * (unsigned)C, (unsigned)chunks);
        if (lds > 32 * 1024)
            if (int rc = allow_large_lds<&k_render_psf_volume_chroma_grad>(kGradLds)) return rc;
        k_render_psf_volume_chroma_grad<<<grid, kBlock, lds, st>>>(img, grad_l, grad_r, tb, B, C, H, W, ks, Dz, Gy, Gx,
                                                                  planes, grad_volume);
    } else {
        const dim3 grid((unsigned)(Gy * Gx), 2u, (unsigned)chunks);
        if (int rc = with_channels(C, [&](auto c) {
                return launch_volume_grad<decltype(c)::value>(grid, lds, st, img, grad_l, grad_r, tb, B, H, W, ks, Dz,
                                                              Gy, Gx, planes, grad_volume);
            }))
            return rc;
    }
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int render_volume_grad_scene(bool chroma, const float* img, const float* volume, const float* grad_l,
                             const float* grad_r, const SegmentTables& tb, int B, int C, int H, int W, int ks, int Dz,
                             int Gy, int Gx, float* grad_img, float* grad_fz, void* stream)
{
    if (!grad_img && !grad_fz) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null pointer (neither gradient is asked for)");
    if (int rc = check_volume_render(img, volume, grad_l, grad_r, tb, B, C, H, W, ks, Dz, Gy, Gx)) return rc;
    if (chroma)
        if (int rc = check_chroma_volume(C, ks, Dz, Gy, Gx)) return rc;
    if (B == 0) return SDIRT_OK;
    const dim3 grid = pixel_grid(B, H, W);
    hipStream_t st = as_stream(stream);
    if (grad_fz) {
        with_channels(C, [&](auto c) {
            constexpr int Cc = decltype(c)::value;
            if (chroma)
                k_render_psf_volume_chroma_grad_depth<Cc><<<grid, kBlock, 0, st>>>(img, volume, grad_l, grad_r, tb, H, W,
                                                                                 ks, Dz, Gy, Gx, grad_fz);
            else
                k_render_psf_volume_grad_depth<Cc><<<grid, kBlock, 0, st>>>(img, volume, grad_l, grad_r, tb, H, W, ks,
                                                                          Dz, Gy, Gx, grad_fz);
            return SDIRT_OK;
        });
        LAUNCH_CHECK();
    }
    if (grad_img) {
        if (chroma) {
            // the channel is a grid dimension: blockIdx.x = c * (16-position chunks of a row) + chunk
            k_render_psf_volume_chroma_grad_img<<<dim3(grid.x * (unsigned)C, grid.y, grid.z), kBlock, 0, st>>>(
                volume, grad_l, grad_r, tb, C, H, W, ks, Dz, Gy, Gx, (int)grid.x, grad_img);
        } else {
            with_channels(C, [&](auto c) {
                k_render_psf_volume_grad_img<decltype(c)::value><<<grid, kBlock, 0, st>>>(volume, grad_l, grad_r, tb, H, W,
                                                                                        ks, Dz, Gy, Gx, grad_img);
                return SDIRT_OK;
            });
        }
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}

}  // namespace

extern "C" {

int sdirt_render_psf_volume(const float* img, const float* volume, const int32_t* ix, const float* fx,
                            const int32_t* iy, const float* fy, const int32_t* iz, const float* fz, int32_t B,
                            int32_t C, int32_t H, int32_t W, int32_t ks, int32_t Dz, int32_t Gy, int32_t Gx,
                            float* out_l, float* out_r, void* stream)
{
    return render_volume(false, img, volume, {ix, fx, iy, fy, iz, fz}, B, C, H, W, ks, Dz, Gy, Gx, out_l, out_r, stream);
}

int sdirt_render_psf_volume_chroma(const float* img, const float* volume, const int32_t* ix, const float* fx,
                                   const int32_t* iy, const float* fy, const int32_t* iz, const float* fz, int32_t B,
                                   int32_t C, int32_t H, int32_t W, int32_t ks, int32_t Dz, int32_t Gy, int32_t Gx,
                                   float* out_l, float* out_r, void* stream)
{
    return render_volume(true, img, volume, {ix, fx, iy, fy, iz, fz}, B, C, H, W, ks, Dz, Gy, Gx, out_l, out_r, stream);
}

int sdirt_render_psf_volume_grad(const float* img, const float* grad_l, const float* grad_r, const int32_t* ix,
                                 const float* fx, const int32_t* iy, const float* fy, const int32_t* iz,
                                 const float* fz, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ks, int32_t Dz,
                                 int32_t Gy, int32_t Gx, float* grad_volume, void* stream)
{
    return render_volume_grad(false, img, grad_l, grad_r, {ix, fx, iy, fy, iz, fz}, B, C, H, W, ks, Dz, Gy, Gx,
                              grad_volume, stream);
}

int sdirt_render_psf_volume_chroma_grad(const float* img, const float* grad_l, const float* grad_r, const int32_t* ix,
                                        const float* fx, const int32_t* iy, const float* fy, const int32_t* iz,
                                        const float* fz, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ks,
                                        int32_t Dz, int32_t Gy, int32_t Gx, float* grad_volume, void* stream)
{
    return render_volume_grad(true, img, grad_l, grad_r, {ix, fx, iy, fy, iz, fz}, B, C, H, W, ks, Dz, Gy, Gx,
                              grad_volume, stream);
}

int sdirt_render_psf_volume_grad_scene(const float* img, const float* volume, const float* grad_l,
                                       const float* grad_r, const int32_t* ix, const float* fx, const int32_t* iy,
                                       const float* fy, const int32_t* iz, const float* fz, int32_t B, int32_t C,
                                       int32_t H, int32_t W, int32_t ks, int32_t Dz, int32_t Gy, int32_t Gx,
                                       float* grad_img, float* grad_fz, void* stream)
{
    return render_volume_grad_scene(false, img, volume, grad_l, grad_r, {ix, fx, iy, fy, iz, fz}, B, C, H, W, ks, Dz, Gy,
                                    Gx, grad_img, grad_fz, stream);
}

int sdirt_render_psf_volume_chroma_grad_scene(const float* img, const float* volume, const float* grad_l,
                                              const float* grad_r, const int32_t* ix, const float* fx,
                                              const int32_t* iy, const float* fy, const int32_t* iz, const float* fz,
                                              int32_t B, int32_t C, int32_t H, int32_t W, int32_t ks, int32_t Dz,
                                              int32_t Gy, int32_t Gx, float* grad_img, float* grad_fz, void* stream)
{
    return render_volume_grad_scene(true, img, volume, grad_l, grad_r, {ix, fx, iy, fy, iz, fz}, B, C, H, W, ks, Dz, Gy,
                                    Gx, grad_img, grad_fz, stream);
}

}  // extern "C"
