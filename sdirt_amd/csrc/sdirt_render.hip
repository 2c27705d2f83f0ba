// sdirt_render.hip -- per-pixel PSF convolution kernels of libsdirt_dp.so (MI355X / gfx950 only):
// local_psf_render / local_psf_render_fast / local_dp_psf_render (deeplens/render_psf.py:76-188)
// and PSFNet.pred + render fused over the network's raw outputs (deeplens/psfnet.py:317-336).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/sdirt_dp.h"
#include "sdirt_device.hpp"
#include "sdirt_host.hpp"
#include "sdirt_render.hpp"

using namespace sdirt;

// ---------------------------------------------------------------------------
// per-pixel PSF convolution (render_psf.py:76-188)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float round_half(float v) { return (float)(_Float16)v; }

// The fp16 arithmetic of the reference's _fast renderer (x.half() * psf.half(), summed in fp32)
// on packed registers: (wl, wr) rounded to fp16 as a pair, one v_pk_mul_f16 per image value --
// the fp16 product of two fp16 numbers IS round_half(float(v) * float(w)): their exact product
// has 22 significant bits and fits fp32 -- and the two widening accumulations.
typedef _Float16 hpair __attribute__((ext_vector_type(2)));
__device__ __forceinline__ hpair half_pair(float lo, float hi) { return hpair{(_Float16)lo, (_Float16)hi}; }
// acc += float(low / high half of the packed pair p), one v_fma_mix_f32 each (the compiler
// splits fma(x, 1, acc) into a conversion and an addition)
__device__ __forceinline__ void acc_halves(hpair p, float& accl, float& accr)
{
    asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(accl) : "v"(p));
    asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(accr) : "v"(p));
}
__device__ __forceinline__ void mul_acc_half(float v, hpair w, float& accl, float& accr)
{
    const _Float16 vh = (_Float16)v;
    acc_halves(hpair{vh, vh} * w, accl, accr);
}
// the same with the image value already rounded to fp16 (the pipelined kernel keeps its patch so)
__device__ __forceinline__ void mul_acc_half(_Float16 vh, hpair w, float& accl, float& accr)
{
    acc_halves(hpair{vh, vh} * w, accl, accr);
}

// Lanes tile a kernel's taps as (rows_per_iter x ks): no integer division inside the tap loops,
// consecutive lanes read consecutive taps (and consecutive image columns).  In step (i0, j0) the lane
// holds tap (i0 + row, j0 + col); beyond 64 columns a kernel row takes several steps of j0.
struct TapTile {
    int rows_per_iter, row, col;
    __device__ __forceinline__ TapTile(int lane, int ks)
        : rows_per_iter(ks <= 64 ? 64 / ks : 1), row(ks <= 64 ? lane / ks : 0), col(ks <= 64 ? lane - row * ks : lane) {}
    __device__ __forceinline__ bool holds(int fi, int fj, int ks) const { return row < rows_per_iter && fi < ks && fj < ks; }
};

// One tap on the C channels of one image position (channel c at px[c * stride]): the fp16
// arithmetic above, or fp32.
template <int C, bool HALF, class Stride>
__device__ __forceinline__ void tap_acc(const float* px, Stride stride, float wl, float wr, float (&accl)[C],
                                        float (&accr)[C])
{
    const hpair wpair = half_pair(wl, wr);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = px[c * stride];
        if (HALF) {
            mul_acc_half(v, wpair, accl[c], accr[c]);
        } else {
            accl[c] += v * wl;
            accr[c] += v * wr;
        }
    }
}

// One WAVE per output pixel: the 64 lanes stride over the 2*ks*ks kernel taps of that
// pixel, so the per-pixel PSFs -- the only large operand, 2*ks*ks*4 B per pixel, read exactly
// once -- stream in as fully coalesced 256-B segments.  The image (a few MB) is gathered
// through L1/L2 with replicate padding (clamped coordinates) and the flipped-tap index of
// render_psf.py:138.  Each lane keeps C partial sums for L and for R; a butterfly of wave
// shuffles reduces them.  A workgroup of 4 waves walks 4 consecutive pixels at a time.
template <int C, bool HALF>
__global__ void __launch_bounds__(kBlock)
k_local_psf_render(const float* __restrict__ img, const float* __restrict__ psf, int B, int H, int W,
                   int ks, float* __restrict__ outl, float* __restrict__ outr)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t P = (int64_t)B * HW;
    const int lane = threadIdx.x & 63;
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const TapTile tile(lane, ks);
    for (int64_t p = wave0; p < P; p += nwaves) {
        const int b = (int)(p / HW);
        const int64_t q = p - (int64_t)b * HW;
        const int y = (int)(q / W), x = (int)(q - (int64_t)y * W);
        const float* kl = psf + p * 2 * kk;
        const float* kr = kl + kk;
        float accl[C], accr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { accl[c] = 0.0f; accr[c] = 0.0f; }
        for (int i0 = 0; i0 < ks; i0 += tile.rows_per_iter) {
            for (int j0 = 0; j0 < ks; j0 += 64) {
                const int fi = i0 + tile.row, fj = j0 + tile.col;
                if (tile.holds(fi, fj, ks)) {
                    const int f = fi * ks + fj;
                    // stored tap f multiplies the neighbour at the FLIPPED offset (render_psf.py:138)
                    const int yy = min(max(y + (ks - 1 - fi) - pad, 0), H - 1);
                    const int xx = min(max(x + (ks - 1 - fj) - pad, 0), W - 1);
                    tap_acc<C, HALF>(img + ((int64_t)b * C * H + yy) * W + xx, HW, kl[f], kr[f], accl, accr);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float a = accl[c], r = accr[c];
            for (int off = 32; off > 0; off >>= 1) {
                a += __shfl_xor(a, off);
                r += __shfl_xor(r, off);
            }
            if (lane == 0) {
                const int64_t o = ((int64_t)(b * C + c) * H + y) * W + x;
                outl[o] = HALF ? round_half(a) : a;
                outr[o] = HALF ? round_half(r) : r;
            }
        }
    }
}

// Sums with DPP row operations (VALU only: no LDS traffic, no address registers).
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xF, false));
}
// every lane of a 16-lane row ends up with the row's sum
__device__ __forceinline__ float row_sum(float v)
{
    v = dpp_add<0xB1>(v);       // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);       // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);      // row_half_mirror
    return dpp_add<0x140>(v);   // row_mirror
}
// the sum over the 64 lanes of a wave, returned in every lane
__device__ __forceinline__ float wave_sum(float v)
{
    v = row_sum(v);
    v = dpp_add<0x142, 0xA>(v);     // row_bcast:15 -> rows 1 and 3 add the previous row
    v = dpp_add<0x143, 0xC>(v);     // row_bcast:31 -> rows 2 and 3 add rows 0+1
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Epilogue of the LDS-tiled kernels: per channel the wave's sums, stored by lane 0 (as fp16 values if HALF).
template <int C, bool HALF>
__device__ __forceinline__ void store_wave_sums(const float (&accl)[C], const float (&accr)[C], int lane, int b, int y,
                                                int x, int H, int W, float* __restrict__ outl,
                                                float* __restrict__ outr)
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a = wave_sum(accl[c]), rr = wave_sum(accr[c]);
        if (lane == 0) {
            const int64_t o = ((int64_t)(b * C + c) * H + y) * W + x;
            outl[o] = HALF ? round_half(a) : a;
            outr[o] = HALF ? round_half(rr) : rr;
        }
    }
}

// LDS-tiled renderer for any kernel size up to 64 and 1 / 3 / 4 channels: a workgroup streams the
// [L | R] kernels of PIX consecutive pixels of one image row (one contiguous run of PIX*2*ks*ks
// floats) into LDS with 16-byte loads -- every PSF byte is read from HBM exactly once, at full
// coalescing width -- then each wave convolves PIX/4 of those pixels reading its weights from LDS.
// blockIdx.y is an image row (b * H + y), blockIdx.x strides over that row's pixel groups.
// Round 1's kernel walked a flat pixel index and paid a 64-bit division per pixel to recover
// (b, y, x) -- a software sequence of ~150 scalar and vector instructions, a third of its
// instruction stream.  Here (b, y) cost one 32-bit division per workgroup, the tap geometry of a
// lane (its row / column inside the kernel, its flipped offsets, its LDS index) is computed once,
// and the per-tap work is: one clamp of the row coordinate, one address, C image gathers, two LDS
// reads, the fp16 arithmetic.  The group's [L | R] kernels are one contiguous run of the PSF
// tensor; it is copied with 16-byte loads whatever its alignment (the LDS image is shifted by the
// run's misalignment so that source and destination stay congruent modulo 16 bytes).
template <int C, bool HALF, int PIX>
__global__ void __launch_bounds__(kBlock)
k_local_psf_render_rows(const float* __restrict__ img, const float* __restrict__ psf, int H, int W,
                        int ks, float* __restrict__ outl, float* __restrict__ outr)
{
    __builtin_assume(ks <= 64);                                      // on this path (a tile of two pixels fits LDS)
    extern __shared__ __attribute__((aligned(16))) float wts[];     // 4 + [PIX][2][ks*ks]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kk = ks * ks;
    const int row = blockIdx.y;
    const int b = row / H, y = row - b * H;
    const int HW = H * W;
    const float* __restrict__ img_b = img + (int64_t)b * C * HW;
    const TapTile tile(lane, ks);
    const bool lane_on = tile.row < tile.rows_per_iter;
    const int pad = (ks - 1) / 2;
    const int dx = (ks - 1 - tile.col) - pad, dy0 = (ks - 1 - tile.row) - pad;     // flipped tap -> neighbour offset
    const int f0 = tile.row * ks + tile.col;
    const int groups = (W + PIX - 1) / PIX;
    typedef float fl4 __attribute__((ext_vector_type(4)));
    for (int gx = blockIdx.x; gx < groups; gx += gridDim.x) {
        const int x0 = gx * PIX;
        const int npix = min(PIX, W - x0);
        const int64_t first = ((int64_t)row * W + x0) * 2 * kk;       // first float of the run
        const int nfl = npix * 2 * kk;
        const int sh = (int)(first & 3);                              // misalignment, in floats
        const float* src = psf + first;
        float* dst = wts + sh;
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
        for (int i = head + (nf4 << 2) + threadIdx.x; i < nfl; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
        for (int q = wave; q < npix; q += kBlock / 64) {
            const int x = x0 + q;
            const int xx = min(max(x + dx, 0), W - 1);
            const float* kl = dst + q * 2 * kk + f0;
            float accl[C], accr[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { accl[c] = 0.0f; accr[c] = 0.0f; }
            for (int i0 = 0; i0 < ks; i0 += tile.rows_per_iter) {
                if (lane_on && i0 + tile.row < ks) {
                    const int yy = min(max(y + dy0 - i0, 0), H - 1);
                    tap_acc<C, HALF>(img_b + (yy * W + xx), HW, kl[i0 * ks], kl[kk + i0 * ks], accl, accr);
                }
            }
            store_wave_sums<C, HALF>(accl, accr, lane, b, y, x, H, W, outl, outr);
        }
        __syncthreads();
    }
}

// Six wave sums for the price of two.  A butterfly level that pairs lanes l and l^16 / l^32 is a
// gfx950 half-exchange (v_permlane16_swap / v_permlane32_swap: the odd rows / the upper half of
// one register trade places with the even rows / the lower half of another) plus ONE addition
// for TWO vectors, whose sums end up in different rows of the result: after both levels
// `q` holds, per 16-lane row, the partial sums of (a0, a1, a2, b0) and `s` those of (b1, b2, b1, b2);
// four DPP additions inside the rows finish both.  19 vector instructions for six sums, against
// 6 x (6 DPP additions + v_readlane).  Row r of q / s: every lane holds the total.
__device__ __forceinline__ float swap16_add(float a, float b)
{
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);   // rows: a(0+1) b(0+1) a(2+3) b(2+3)
}
__device__ __forceinline__ float swap32_add(float a, float b)
{
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);   // lanes 0-31: a(lo+hi), 32-63: b(lo+hi)
}
__device__ __forceinline__ void wave_sum6(const float (&a)[3], const float (&b)[3], float& q, float& s)
{
    const float p01 = swap16_add(a[0], a[1]), p23 = swap16_add(a[2], b[0]), p45 = swap16_add(b[1], b[2]);
    q = row_sum(swap32_add(p01, p23));          // rows: a0 a1 a2 b0
    s = row_sum(swap32_add(p45, p45));          // rows: b1 b2 b1 b2
}


// ---------------------------------------------------------------------------
// one wave per pixel, weights straight from HBM into registers (ks 21, RGB)
// ---------------------------------------------------------------------------
// (Round 2's first version moved every weight through LDS -- 16-byte loads, a write, a read per
// weight, two barriers per 8 pixels -- and spent 165 instructions per pixel and wave.)  Here lane l
// loads the weights of ITS taps (f = 64 it + l: consecutive lanes, consecutive values -- each load
// instruction of a wave is one contiguous run of the pixel's kernel) one pixel ahead of the
// one being convolved; LDS holds only the image patch of the workgroup's CHUNK-pixel stretch of
// the row ([KS][CHUNK + KS - 1] positions x 4 channel slots: one 8- or 16-byte read per tap gives
// all channels), staged once: one barrier per workgroup, none around the weights.  The six sums
// of a pixel are reduced together (wave_sum6) and stored by 4 + 2 lanes in two instructions.
//
// Where a lane's weights come from is a tap source `Taps`: its element types (WeightT in registers,
// PatchT in LDS), whether results are fp16 values (HALF), load() of one pixel's raw weights and
// weights() from raw to the fp32 factors of the taps, zero in the lanes past the last tap.
// The geometry, used by the body and by the launchers:
template <class Taps, int CHUNK>
struct WaveGeom {
    static constexpr int KS = Taps::KS, kk = KS * KS, pad = (KS - 1) / 2;
    static constexpr int PW = CHUNK + KS - 1;               // patch width
    static constexpr int NI = Taps::NI;                     // taps per lane
    static constexpr int NPOS = KS * PW;                    // patch positions
    static constexpr int NQ = (NPOS + kBlock - 1) / kBlock;
    static constexpr int NW = kBlock / 64, PPW = CHUNK / NW;   // waves, pixels per wave
    static constexpr size_t lds_bytes = (size_t)NPOS * 4 * sizeof(typename Taps::PatchT);   // 4 channel slots
    static dim3 grid(int B, int H, int W) { return dim3((unsigned)((W + CHUNK - 1) / CHUNK), (unsigned)(B * H)); }
};

// what every tap source knows about its lane: the lanes past the last tap (448 - 441 at ks 21) read tap kk-1
template <int KS_>
struct LaneTaps {
    static constexpr int KS = KS_, kk = KS * KS, NI = (kk + 63) / 64;
    const int lane, W, ftail;
    const bool tail_on;
    __device__ __forceinline__ LaneTaps(int lane_, int W_)
        : lane(lane_), W(W_), ftail(min((NI - 1) * 64 + lane_, kk - 1)), tail_on((NI - 1) * 64 + lane_ < kk) {}
    __device__ __forceinline__ bool on(int it) const { return it + 1 < NI || tail_on; }
};

// fp32 kernel pairs [row][x][2][kk], as they are: no normalisation, fp16 arithmetic only if HALF
template <bool HALF_, int KS_>
struct PsfTaps : LaneTaps<KS_> {
    using LaneTaps<KS_>::NI; using LaneTaps<KS_>::kk;
    static constexpr bool HALF = HALF_;
    typedef float WeightT;
    typedef typename std::conditional<HALF, _Float16, float>::type PatchT;
    const float* __restrict__ wrow;                          // this image row's kernels
    __device__ __forceinline__ PsfTaps(const float* psf, int row, int W_, int lane_)
        : LaneTaps<KS_>(lane_, W_), wrow(psf + (int64_t)row * W_ * 2 * kk) {}
    __device__ __forceinline__ void load(int x, float (&l)[NI], float (&r)[NI]) const
    {
        const float* __restrict__ k0 = wrow + (int64_t)min(x, this->W - 1) * 2 * kk + this->lane;
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int f = it + 1 < NI ? it * 64 : this->ftail - this->lane;
            l[it] = __builtin_nontemporal_load(k0 + f);
            r[it] = __builtin_nontemporal_load(k0 + kk + f);
        }
    }
    __device__ __forceinline__ void weights(const float (&l)[NI], const float (&r)[NI], float (&wl)[NI],
                                            float (&wr)[NI]) const
    {
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            wl[it] = this->on(it) ? l[it] : 0.0f;
            wr[it] = this->on(it) ? r[it] : 0.0f;
        }
    }
};

// PSFNet.pred (psfnet.py:317-336) on the network's raw fp16 outputs [row][x][kk]: the right kernel through the
// fliplr'ed tap (psfnet.py:330 -- a permutation of the taps, so its values also make up the right kernel's
// sum), both kernels divided by their sums
template <int KS_>
struct RawNetTaps : LaneTaps<KS_> {
    using LaneTaps<KS_>::NI; using LaneTaps<KS_>::kk; using LaneTaps<KS_>::KS;
    static constexpr bool HALF = true;
    typedef _Float16 WeightT;
    typedef _Float16 PatchT;
    const _Float16* __restrict__ lrow;
    const _Float16* __restrict__ rrow;
    int fr[NI];
    __device__ __forceinline__ RawNetTaps(const _Float16* raw_l, const _Float16* raw_r, int row, int W_, int lane_)
        : LaneTaps<KS_>(lane_, W_), lrow(raw_l + (int64_t)row * W_ * kk), rrow(raw_r + (int64_t)row * W_ * kk)
    {
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int f = min(it * 64 + lane_, kk - 1);
            const int fi = f / KS, fj = f - fi * KS;
            fr[it] = fi * KS + (KS - 1 - fj);
        }
    }
    __device__ __forceinline__ void load(int x, _Float16 (&l)[NI], _Float16 (&r)[NI]) const
    {
        const int k0 = min(x, this->W - 1) * kk;       // a row's runs fit 32-bit offsets (checked by the host)
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            l[it] = __builtin_nontemporal_load(lrow + (k0 + (it + 1 < NI ? it * 64 + this->lane : this->ftail)));
            r[it] = __builtin_nontemporal_load(rrow + (k0 + fr[it]));
        }
    }
    __device__ __forceinline__ void weights(const _Float16 (&hl)[NI], const _Float16 (&hr)[NI], float (&wl)[NI],
                                            float (&wr)[NI]) const
    {
        float sl = 0.0f, sr = 0.0f;
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            wl[it] = this->on(it) ? (float)hl[it] : 0.0f;
            wr[it] = this->on(it) ? (float)hr[it] : 0.0f;
            sl += wl[it];
            sr += wr[it];
        }
        // both sums at once: even rows of t end up with sum(sl), odd rows with sum(sr)
        const float t = row_sum(swap32_add(swap16_add(sl, sr), swap16_add(sl, sr)));
        const float tot_l = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 0));
        const float tot_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 16));
        // psf / (psf.sum() + 1e-9) in half precision (psfnet.py:333): the sum rounded to fp16
        const float inv_l = sdirt::Lean::div(1.0f, round_half(tot_l) + 1e-9f);
        const float inv_r = sdirt::Lean::div(1.0f, round_half(tot_r) + 1e-9f);
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            wl[it] *= inv_l;
            wr[it] *= inv_r;
        }
    }
};

template <int C, int CHUNK, class Taps, class... Src>
__device__ __forceinline__ void render_wave(const float* __restrict__ img, int H, int W, float* __restrict__ outl,
                                            float* __restrict__ outr, Src... src)
{
    static_assert(C == 3, "row layout of wave_sum6");
    typedef WaveGeom<Taps, CHUNK> G;
    constexpr int KS = G::KS, pad = G::pad, PW = G::PW, NI = G::NI, NPOS = G::NPOS, NW = G::NW, PPW = G::PPW;
    static_assert(PPW % 2 == 0, "the pixel loop is unrolled by two");
    typedef typename Taps::PatchT PatchT;
    typedef typename Taps::WeightT WeightT;
    typedef PatchT pvec __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    pvec* patch = reinterpret_cast<pvec*>(lds_raw);  // [NPOS]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.y;
    const int b = row / H, y = row - b * H;
    const int HW = H * W;
    const int x0 = blockIdx.x * CHUNK;
    const Taps taps(src..., row, W, lane);
    WeightT wa[NI], ra[NI], wb[NI], rb[NI];
    taps.load(x0 + wave, wa, ra);                    // in flight while the patch is staged
    {
        const float* __restrict__ img_b = img + (int64_t)b * C * HW;
#pragma unroll
        for (int u = 0; u < G::NQ; ++u) {
            const int e = threadIdx.x + u * kBlock;
            if (e < NPOS) {
                const int r = e / PW, col = e - r * PW - pad;
                const int o = min(max(y + r - pad, 0), H - 1) * W + min(max(x0 + col, 0), W - 1);
                pvec v;
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = (PatchT)img_b[c * HW + o];
                v[3] = (PatchT)0.0f;
                patch[e] = v;
            }
        }
    }
    // tap f = 64 it + l of the kernel multiplies the neighbour at the flipped offset
    // (render_psf.py:138): patch row KS-1-fi, patch column q + KS-1-fj
    int ptap[NI];
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int f = min(it * 64 + lane, G::kk - 1);
        const int fi = f / KS, fj = f - fi * KS;
        ptap[it] = (KS - 1 - fi) * PW + (KS - 1 - fj);
    }
    // this lane's output slot: rows 0..2 of the reduced vector q are the L channels, row 3 is R
    // channel 0; rows 0, 1 of s are R channels 1, 2
    const int r16 = lane >> 4;
    float* __restrict__ oq = (r16 < 3 ? outl + ((int64_t)(b * C + r16) * H + y) * W
                                      : outr + ((int64_t)(b * C) * H + y) * W);
    float* __restrict__ os = outr + ((int64_t)(b * C + 1 + (r16 & 1)) * H + y) * W;
    const bool store_q = (lane & 15) == 0, store_s = (lane & 47) == 0;
    __syncthreads();

    auto pixel = [&](int x, const WeightT (&l)[NI], const WeightT (&r)[NI]) {
        if (x >= W) return;
        const pvec* pp = patch + (x - x0);
        float wl[NI], wr[NI];
        taps.weights(l, r, wl, wr);
        float accl[C], accr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { accl[c] = 0.0f; accr[c] = 0.0f; }
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const pvec v = pp[ptap[it]];
            if (Taps::HALF) {
                const hpair wpair = half_pair(wl[it], wr[it]);
#pragma unroll
                for (int c = 0; c < C; ++c) mul_acc_half((_Float16)v[c], wpair, accl[c], accr[c]);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    accl[c] += (float)v[c] * wl[it];
                    accr[c] += (float)v[c] * wr[it];
                }
            }
        }
        float q, s2;
        wave_sum6(accl, accr, q, s2);
        if (Taps::HALF) { q = round_half(q); s2 = round_half(s2); }
        if (store_q) oq[x] = q;
        if (store_s) os[x] = s2;
    };
#pragma unroll 1
    for (int j = 0; j < PPW; j += 2) {
        const int x = x0 + wave + j * NW;
        taps.load(x + NW, wb, rb);
        pixel(x, wa, ra);
        if (j + 2 < PPW) taps.load(x + 2 * NW, wa, ra);
        pixel(x + NW, wb, rb);
    }
}

template <int C, bool HALF, int KS, int CHUNK>
__global__ void __launch_bounds__(kBlock)
k_local_psf_render_wave(const float* __restrict__ img, const float* __restrict__ psf, int H, int W,
                        float* __restrict__ outl, float* __restrict__ outr)
{
    render_wave<C, CHUNK, PsfTaps<HALF, KS>>(img, H, W, outl, outr, psf);
}

// PSFNet.pred + local_psf_render_fast in one pass, wave per pixel: see k_psfnet_render below, whose results
// this kernel's equal up to the order of the fp32 sums.
template <int C, int KS, int CHUNK>
__global__ void __launch_bounds__(kBlock)
k_psfnet_render_wave(const float* __restrict__ img, const _Float16* __restrict__ raw_l,
                     const _Float16* __restrict__ raw_r, int H, int W,
                     float* __restrict__ outl, float* __restrict__ outr)
{
    render_wave<C, CHUNK, RawNetTaps<KS>>(img, H, W, outl, outr, raw_l, raw_r);
}

// PSFNet.pred (psfnet.py:317-336) + local_psf_render_fast (render_psf.py:120-155) in one pass
// over the network's raw fp16 outputs: raw_l = net(x, y, z), raw_r = net(-x, y, z), both
// [P, ks*ks].  Per pixel: L taps = raw_l / (sum(raw_l) + 1e-9), R taps = fliplr(raw_r) /
// (sum(raw_r) + 1e-9), then the per-pixel convolution with the fp16 arithmetic of the _fast
// renderer.  The stacked / flipped / normalised [P,2,ks,ks] tensor the reference materialises
// (and re-reads twice) never exists: each raw value is read from HBM once, as fp16.
// A zero-sum kernel renders 0 (the reference's fp16 division would give NaN there).
template <int C, int PIX, int KS>
__global__ void __launch_bounds__(kBlock)
k_psfnet_render(const float* __restrict__ img, const _Float16* __restrict__ raw_l,
                const _Float16* __restrict__ raw_r, int B, int H, int W, int ks_rt,
                float* __restrict__ outl, float* __restrict__ outr)
{
    const int ks = KS > 0 ? KS : ks_rt;
    extern __shared__ __attribute__((aligned(16))) _Float16 wh[];   // [2][PIX][ks*ks]
    const int64_t HW = (int64_t)H * W;
    const int64_t P = (int64_t)B * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pad = (ks - 1) / 2, kk = ks * ks;
    const TapTile tile(lane, ks);
    const int64_t ngroups = (P + PIX - 1) / PIX;
    typedef float fl4 __attribute__((ext_vector_type(4)));
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t p0 = g * PIX;
        const int npix = (int)min((int64_t)PIX, P - p0);
        const int nh = npix * kk;                                   // halves per side
        const int nv = nh >> 3;                                     // 16-byte vectors per side
        // PIX is a multiple of 8, so both runs start 16-byte aligned
        const fl4* sl4 = reinterpret_cast<const fl4*>(raw_l + p0 * kk);
        const fl4* sr4 = reinterpret_cast<const fl4*>(raw_r + p0 * kk);
        fl4* dl4 = reinterpret_cast<fl4*>(wh);
        fl4* dr4 = reinterpret_cast<fl4*>(wh + PIX * kk);
        constexpr int STAGE_U = 4;
        for (int base = threadIdx.x; base < nv; base += kBlock * STAGE_U) {
            fl4 a[STAGE_U], b[STAGE_U];
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u)
                if (base + u * kBlock < nv) {
                    a[u] = __builtin_nontemporal_load(&sl4[base + u * kBlock]);
                    b[u] = __builtin_nontemporal_load(&sr4[base + u * kBlock]);
                }
#pragma unroll
            for (int u = 0; u < STAGE_U; ++u)
                if (base + u * kBlock < nv) { dl4[base + u * kBlock] = a[u]; dr4[base + u * kBlock] = b[u]; }
        }
        for (int i = (nv << 3) + threadIdx.x; i < nh; i += blockDim.x) {
            wh[i] = raw_l[p0 * kk + i];
            wh[PIX * kk + i] = raw_r[p0 * kk + i];
        }
        __syncthreads();
        for (int q = wave; q < npix; q += kBlock / 64) {
            const int64_t p = p0 + q;
            const int b = (int)(p / HW);
            const int64_t r = p - (int64_t)b * HW;
            const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
            const _Float16* kl = wh + q * kk;
            const _Float16* kr = wh + PIX * kk + q * kk;
            float sl = 0.0f, sr = 0.0f;
            for (int f = lane; f < kk; f += 64) { sl += (float)kl[f]; sr += (float)kr[f]; }
            const float inv_l = 1.0f / (round_half(wave_sum(sl)) + 1e-9f);
            const float inv_r = 1.0f / (round_half(wave_sum(sr)) + 1e-9f);
            float accl[C], accr[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { accl[c] = 0.0f; accr[c] = 0.0f; }
#pragma unroll KS > 0 ? 8 : 1
            for (int i0 = 0; i0 < ks; i0 += tile.rows_per_iter) {
                for (int j0 = 0; j0 < ks; j0 += 64) {
                    const int fi = i0 + tile.row, fj = j0 + tile.col;
                    if (tile.holds(fi, fj, ks)) {
                        const int yy = min(max(y + (ks - 1 - fi) - pad, 0), H - 1);
                        const int xx = min(max(x + (ks - 1 - fj) - pad, 0), W - 1);
                        tap_acc<C, true>(img + ((int64_t)b * C * H + yy) * W + xx, HW, (float)kl[fi * ks + fj] * inv_l,
                                         (float)kr[fi * ks + (ks - 1 - fj)] * inv_r, accl, accr);
                    }
                }
            }
            store_wave_sums<C, true>(accl, accr, lane, b, y, x, H, W, outl, outr);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
namespace {

constexpr int kChunk = 64;      // pixels of a row per workgroup of the wave-per-pixel kernels

struct RenderCall {
    const float* img;
    int B, H, W, ks;
    float* out_l;
    float* out_r;
    hipStream_t st;
    int64_t pixels() const { return (int64_t)B * H * W; }
};

template <int C, bool HALF, int PIX>
int launch_rows(const RenderCall& r, const float* psf, size_t per_pixel)
{
    const size_t lds_tile = per_pixel * PIX + 16;
    const int groups = (r.W + PIX - 1) / PIX;
    // ~16 workgroups per CU in flight; the rest of a row's groups are walked by the same workgroup
    const int64_t rows = (int64_t)r.B * r.H;
    const int gx = std::max(1, std::min(groups, (int)((256 * 16 + rows - 1) / rows)));
    if (lds_tile > 48 * 1024)
        if (int rc = allow_large_lds<&k_local_psf_render_rows<C, HALF, PIX>>(64 * 1024)) return rc;
    k_local_psf_render_rows<C, HALF, PIX><<<dim3((unsigned)gx, (unsigned)rows), kBlock, lds_tile, r.st>>>(
        r.img, psf, r.H, r.W, r.ks, r.out_l, r.out_r);
    return SDIRT_OK;
}

// pix: how many pixels' kernels the row-mapped LDS-tiled kernel holds at a time, 0 for the direct kernel
template <int C, bool HALF>
int launch_render(const RenderCall& r, const float* psf, size_t per_pixel, int pix)
{
    // the reference's PSFNet kernel size (configs/dfdp_by_sdirt_rf50mm.yml: ks 21) on RGB: one workgroup per
    // 64-pixel stretch of a row, LDS = the stretch's image patch (14 KB fp16 / 28 KB fp32)
    if (pix == 8 && r.ks == 21 && C == 3) {
        typedef WaveGeom<PsfTaps<HALF, 21>, kChunk> G;
        k_local_psf_render_wave<3, HALF, 21, kChunk><<<G::grid(r.B, r.H, r.W), kBlock, G::lds_bytes, r.st>>>(
            r.img, psf, r.H, r.W, r.out_l, r.out_r);
        return SDIRT_OK;
    }
    switch (pix) {
    case 8: return launch_rows<C, HALF, 8>(r, psf, per_pixel);
    case 4: return launch_rows<C, HALF, 4>(r, psf, per_pixel);
    case 2: return launch_rows<C, HALF, 2>(r, psf, per_pixel);
    }
    const int grid = grid_for(r.pixels() * 64, kBlock, 256 * 32);      // one wave per pixel, grid-stride
    k_local_psf_render<C, HALF><<<grid, kBlock, 0, r.st>>>(r.img, psf, r.B, r.H, r.W, r.ks, r.out_l, r.out_r);
    return SDIRT_OK;
}

template <int C, int PIX, int KS>
int launch_psfnet_tiles(const RenderCall& r, const _Float16* rl, const _Float16* rr, size_t per_pixel)
{
    const size_t lds = per_pixel * PIX;
    const int grid = (int)std::min<int64_t>((r.pixels() + PIX - 1) / PIX, 256 * 64);
    if (lds > 48 * 1024)
        if (int rc = allow_large_lds<&k_psfnet_render<C, PIX, KS>>(64 * 1024)) return rc;
    k_psfnet_render<C, PIX, KS><<<grid, kBlock, lds, r.st>>>(r.img, rl, rr, r.B, r.H, r.W, r.ks, r.out_l, r.out_r);
    return SDIRT_OK;
}

template <int C>
int launch_psfnet(const RenderCall& r, const _Float16* rl, const _Float16* rr, size_t per_pixel)
{
    if (r.ks == 21 && C == 3) {
        if ((int64_t)3 * r.H * r.W < (1ll << 30) && (int64_t)r.B * r.H < 65536) {
            typedef WaveGeom<RawNetTaps<21>, kChunk> G;
            k_psfnet_render_wave<3, 21, kChunk><<<G::grid(r.B, r.H, r.W), kBlock, G::lds_bytes, r.st>>>(
                r.img, rl, rr, r.H, r.W, r.out_l, r.out_r);
            return SDIRT_OK;
        }
        return launch_psfnet_tiles<3, 16, 21>(r, rl, rr, per_pixel);
    }
    if (per_pixel * 16 <= 32 * 1024) return launch_psfnet_tiles<C, 16, 0>(r, rl, rr, per_pixel);
    return launch_psfnet_tiles<C, 8, 0>(r, rl, rr, per_pixel);
}

}  // namespace

extern "C" {

int sdirt_local_psf_render(const float* img, const float* psf, int32_t B, int32_t C, int32_t H,
                           int32_t W, int32_t ks, int32_t half_precision, float* out_l, float* out_r,
                           void* stream)
{
    // no limit on ks, B or H here (the direct kernel takes any), C is refused at the dispatch
    if (int rc = check_image_call({img, psf, out_l, out_r}, B, C, H, W, ks, 0, false)) return rc;
    if (B == 0) return SDIRT_OK;
    const RenderCall r{img, B, H, W, ks, out_l, out_r, as_stream(stream)};
    // row-mapped LDS-tiled kernel whenever 8 (or 4, or 2) pixels' kernels fit in 64 KB of LDS and the
    // image fits 32-bit offsets, else the direct one-wave-per-pixel kernel
    const size_t per_pixel = sizeof(float) * 2 * (size_t)ks * ks;
    const bool small = ks <= 64 && (int64_t)C * H * W < (1ll << 30) && (int64_t)B * H < 65536;
    const int pix = !small ? 0 : per_pixel * 8 + 16 <= 64 * 1024 ? 8 : per_pixel * 4 + 16 <= 64 * 1024 ? 4
                    : per_pixel * 2 + 16 <= 64 * 1024 ? 2 : 0;
    const int rc = with_channels(C, [&](auto c) {
        return with_bool(half_precision != 0, [&](auto half) {
            return launch_render<decltype(c)::value, decltype(half)::value>(r, psf, per_pixel, pix);
        });
    });
    if (rc) return rc;
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_psfnet_render(const float* img, const void* raw_l, const void* raw_r, int32_t B, int32_t C,
                        int32_t H, int32_t W, int32_t ks, float* out_l, float* out_r, void* stream)
{
    if (int rc = check_image_call({img, raw_l, raw_r, out_l, out_r}, B, C, H, W, ks, 0, false)) return rc;
    if (((uintptr_t)raw_l | (uintptr_t)raw_r) & 15)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "raw_l / raw_r must be 16-byte aligned");
    if (B == 0) return SDIRT_OK;
    const RenderCall r{img, B, H, W, ks, out_l, out_r, as_stream(stream)};
    const size_t per_pixel = sizeof(_Float16) * 2 * (size_t)ks * ks;
    if (per_pixel * 8 > 64 * 1024)
        return fail(SDIRT_ERR_UNSUPPORTED, "ks=%d: eight pixels' kernels exceed 64 KB of LDS", ks);
    const _Float16* rl = static_cast<const _Float16*>(raw_l);
    const _Float16* rr = static_cast<const _Float16*>(raw_r);
    const int rc = with_channels(C, [&](auto c) { return launch_psfnet<decltype(c)::value>(r, rl, rr, per_pixel); });
    if (rc) return rc;
    LAUNCH_CHECK();
    return SDIRT_OK;
}

}  // extern "C"
