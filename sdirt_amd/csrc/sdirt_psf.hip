// sdirt_psf.hip -- the PSF kernels of libsdirt_dp.so (MI355X / gfx950 only): forward_integral on
// staged rays, max-normalisation, the fused chief-ray centre, and k_psf_lr = [chief-ray pass ->]
// sample -> trace -> propagate -> window -> dual-pixel weights -> LDS splat -> normalise -> store
// (deeplens/optics.py:889-996, deeplens/monte_carlo.py:9-372).  See include/sdirt_dp.h for the
// ABI and DESIGN.md for the data layout and the roofline of each kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/sdirt_dp.h"
#include "sdirt_trace.hpp"

using namespace sdirt;

// Everything the splat of one ray needs (window geometry + dual-pixel parameters), as ONE
// 64-byte block at offset 0 of k_psf_lr's kernel-argument segment: the kernel fetches it with one
// scalar load per RAY, right before the splat, instead of keeping ~20 SGPRs alive through the
// trace (where round 1's build parked them in VGPR lanes: v_writelane / v_readlane traffic).
// Words 7..14 are the dual-pixel parameters of the closed form -- or, in the TAB instantiations, which never
// evaluate it, the reference to the sensor's weight table (DpTableRef): the pointer travels in the block the
// kernel re-reads per ray and costs no SGPR across the trace.
struct alignas(64) SplatBlock {
    float lim, x_min, y_max, dx_rng, dy_rng, ksm1;
    int32_t ks;
    union {
        struct { float h, f, w, r, fmh, rr, inv_r; int32_t r_pow2; } dp;                    // words 7..14
        struct { float scale; uint32_t tab_lo, tab_hi; float lo, hi; int32_t half; float h, w; } tb;   // 7, 8-9 (pointer), 10 .. 14
    };
    int32_t pad;
};
static_assert(sizeof(SplatBlock) == 64, "layout");
static_assert(offsetof(SplatBlock, dp.h) == 28 && offsetof(SplatBlock, dp.r_pow2) == 56, "layout");
static_assert(offsetof(SplatBlock, tb.scale) == 28 && offsetof(SplatBlock, tb.tab_lo) == 32 && offsetof(SplatBlock, tb.half) == 48, "layout");

static SplatBlock make_splat_block(const SplatGeom& g, const DevDpParams& p, const DpTableRef* t)
{
    SplatBlock b;
    std::memset(&b, 0, sizeof(b));
    b.lim = g.lim; b.x_min = g.x_min; b.y_max = g.y_max; b.dx_rng = g.dx_rng; b.dy_rng = g.dy_rng;
    b.ksm1 = g.ksm1; b.ks = g.ks;
    if (t) {
        b.tb.scale = t->scale; b.tb.tab_lo = (uint32_t)(uintptr_t)t->tab; b.tb.tab_hi = (uint32_t)((uintptr_t)t->tab >> 32); b.tb.lo = t->lo; b.tb.hi = t->hi; b.tb.half = t->half;
        b.tb.h = t->h; b.tb.w = t->w;
    } else {
        b.dp.h = p.h; b.dp.f = p.f; b.dp.w = p.w; b.dp.r = p.r; b.dp.fmh = p.fmh; b.dp.rr = p.rr; b.dp.inv_r = p.inv_r;
        b.dp.r_pow2 = p.r_pow2;
    }
    return b;
}

// What k_psf_lr's prologue and epilogue need of the launch -- sample arrays, sizes, planes, strides --, as a SECOND
// 64-byte block, at offset 64 of the kernel-argument segment: one scalar load where the workgroup starts, one more where
// it ends, and nothing of it held in an SGPR across the sample loops.  What a ray needs of it at its ends (its sample
// addresses, the point, the planes, the last sample) is wave-uniform but only ever a VECTOR operand and lives in VGPRs
// (in_vgpr), of which the Lean kernels have ten to spare.  As plain kernel arguments these were SGPRs that the register
// allocator, out of its 80 inside the Newton loops, parked in VGPR lanes: some 65 v_readlane / v_writelane per traced
// ray that compute nothing (docs/KERNEL_NOTES.md, "Lane moves"; `make lanes` counts them).
struct alignas(64) LoopBlock {
    const float* x2;
    const float* y2;
    const float* po;
    int32_t S, chunk, nsplit, K;
    float pz, zs;
    int32_t ks, pstride, prio_from, pad;
};
static_assert(sizeof(LoopBlock) == 64, "layout");
static_assert(offsetof(LoopBlock, x2) == 0 && offsetof(LoopBlock, y2) == 8 && offsetof(LoopBlock, po) == 16, "layout");
static_assert(offsetof(LoopBlock, S) == 24 && offsetof(LoopBlock, K) == 36 && offsetof(LoopBlock, pz) == 40, "layout");
static_assert(offsetof(LoopBlock, ks) == 48 && offsetof(LoopBlock, prio_from) == 56, "layout");

// A wave-uniform value that is only ever a vector operand (an address base, a bound a lane index is compared with, a
// coordinate) in a VGPR: behind this the compiler treats it as a per-lane value and never asks an SGPR for it.
template <class T>
__device__ __forceinline__ T in_vgpr(T v)
{
    asm("" : "+v"(v));
    return v;
}
// ... where the kernel has the VGPRs for it (ON): the strict-IEEE and the big-radius instantiations of k_psf_lr are at
// their VGPR budget and would pay with scratch
template <bool ON, class T>
__device__ __forceinline__ T in_vgpr_if(T v)
{
    if constexpr (ON) return in_vgpr(v);
    else return v;
}
typedef const __attribute__((address_space(1))) float* GlobalF;    // behind in_vgpr the compiler cannot tell any more

// One word of a block that sload_block fetched, as a value of its own: the register allocator otherwise keeps -- and
// parks, and brings back -- all sixteen registers of the block for as long as one of them is in use.
__device__ __forceinline__ uint32_t in_sgpr(uint32_t v)
{
    uint32_t o;
    asm("s_mov_b32 %0, %1" : "=s"(o) : "s"(v));
    return o;
}

// ---------------------------------------------------------------------------
// the sensor's dual-pixel weight table
// ---------------------------------------------------------------------------
// (sl, sr) of monte_carlo.py:169-206 (r <= 0.5) are a function of ONE scalar per ray, x_tan, and of the sensor's
// (h, f, w, r): k_psf_lr's Lean instantiations read their segment-area part (DpTableRef, sdirt_device.hpp) from a
// table of that function instead of evaluating six segment areas per ray (dp_weights_small: ~140 vector
// instructions, six square roots).
//   entries  float64 evaluation of the reference's literal sequence (clamp, acos, u - sin(2u) / 2), rounded to fp32 once
//   spacing  2^-k in x_tan, the largest k whose table fits kDpTableEntries: 2^-16 for the default sensor (134 439
//            entries, 1.03 MiB, L2-resident); a power of two makes x_tan * 2^k exact, so the fraction has no rounding
//   extent   |x_tan| <= X = the point beyond which all six clamped arguments are saturated and the areas are
//            constant, plus two cells; the kernel clamps the index, the end entries ARE the saturated values
//   error    linear interpolation of a C1 function that behaves like (1 - z)^(3/2) at each of its twelve saturation
//            points: a segment area is r^2 S(z) with S -> 1.886 (1 - z)^1.5, and a chord of s^1.5 over a cell d is off
//            by at most 0.148 d^1.5, so the worst error is 0.148 * 1.886 r^2 (z' 2^-k)^1.5 with z' = d z / d x_tan of the
//            steepest abscissa (f h / (f - h) / r through the microlens); a sensor so steep that this exceeds
//            kDpTableErrMax gets no table (2.6e-8 for the default sensor).  Measured against float64 on 2e5 points per
//            parameter set (tests/test_gpu_dp_weight_table.py), with the closed form's own error beside it: see
//            docs/KERNEL_NOTES.md
constexpr double kDpTableErrMax = 1e-7;      // a third of seg_acos's 3.1e-7: entry and interpolation roundings add ~1e-7
struct DpTablePlan {
    double h, f, w, r;
    int half, k;
};
static bool plan_dp_table(const sdirt_dp_params* dp, DpTablePlan& pl)
{
    pl.h = dp ? dp->h : 0.78; pl.f = dp ? dp->f : 1.44; pl.w = dp ? dp->w : 0.3; pl.r = dp ? dp->r : 0.5;
    const double fmh = pl.f - pl.h, rc = std::min(pl.r, 0.5);
    // x_ml: |f h / fmh x| >= r + |w f / fmh| saturates the microlens trio; x_in: |h x| >= |w| + rc the pixel trio
    const double x_ml = (pl.r + std::fabs(pl.w * pl.f / fmh)) / std::fabs(pl.f * pl.h / fmh);
    const double x_in = (std::fabs(pl.w) + rc) / std::fabs(pl.h);
    const double X = std::max(x_ml, x_in);
    if (!(pl.r > 0.0) || pl.r > 0.5 || !std::isfinite(X) || !(X > 0.0)) return false;
    int e = 0;
    (void)std::frexp((kDpTableEntries / 2 - 2) / X, &e);       // (cap - 2) / X in [2^(e-1), 2^e)
    pl.k = e - 1;
    if (pl.k < -24 || pl.k > 24) return false;                  // a sensor outside anything the splat can resolve
    pl.half = (int)std::ceil(std::ldexp(X, pl.k)) + 2;
    const double steep = std::max(std::fabs(pl.f * pl.h / fmh), std::fabs(pl.h)) / pl.r;
    if (!(0.148 * 1.886 * pl.r * pl.r * std::pow(std::ldexp(steep, -pl.k), 1.5) <= kDpTableErrMax)) return false;
    return pl.half >= 2 && pl.half <= kDpTableEntries / 2;
}

__device__ __forceinline__ double seg64(double x, double r)    // rr-less segment area of a clamped abscissa
{
    const double u = acos(x / r);
    return u - 0.5 * sin(2.0 * u);
}
__device__ __forceinline__ double clamp64(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

__global__ void __launch_bounds__(kBlock) k_dp_table_build(float2* __restrict__ tab, int half, double cell, double h, double f,
                                                           double w, double r)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > 2 * half) return;
    const double x = (double)(i - half) * cell, rr = r * r, fmh = f - h;
    const double fx = f * x, hx = h * x;
    double xr = clamp64(w - (fx - w) * h / fmh, -r, r), xm = clamp64((-fx) * h / fmh, -r, r),
           xl = clamp64((-w) - (fx + w) * h / fmh, -r, r);
    double sm = seg64(xm, r);
    const double sr_ml = rr * (sm - seg64(xr, r)), sl_ml = rr * (seg64(xl, r) - sm);
    xr = clamp64(w - hx, -0.5, 0.5); xm = clamp64(-hx, -0.5, 0.5); xl = clamp64((-w) - hx, -0.5, 0.5);
    sm = seg64(clamp64(xm, -r, r), r);
    const double sr_in = rr * (sm - seg64(clamp64(xr, -r, r), r)), sl_in = rr * (seg64(clamp64(xl, -r, r), r) - sm);
    tab[i] = make_float2((float)(sl_ml - sl_in), (float)(sr_ml - sr_in));     // the strip widths xm - xl, xr - xm: in the kernel
}

// The table of `dp` on `lens`, ready for a kernel enqueued on `st` behind this call: the handle's entries when they
// were built from the same bit patterns, else rebuilt on `st` first -- build, then use, in stream order; no host
// synchronisation.  Other streams are ordered by an event: a stream that has not used this build yet waits for it, a
// rebuild waits for every stream that used the entries it overwrites.  false: no table for this call (r > 0.5, a
// degenerate or very steep sensor, a stream that is being captured -- a graph would replay the use without the build) and the
// kernel evaluates the closed form.
// What the caller owes, as for every other field of the handle: calls that render through ONE handle with DIFFERENT
// sensors come from one thread at a time (the lock covers the bookkeeping, not the launch that follows it), and a
// stream that has rendered through the handle outlives it or the next rebuild (the list keeps its handle).
static bool dp_table_for(const sdirt_lens* lens, const sdirt_dp_params* dp, hipStream_t st, DpTableRef& ref)
{
    DpWeightTable& T = lens->dp_table;
    DpTablePlan pl;
    if (!T.dev || !T.ready || !plan_dp_table(dp, pl)) return false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return false;
    }
    uint64_t key[4];
    const double v[4] = {pl.h, pl.f, pl.w, pl.r};
    std::memcpy(key, v, sizeof(key));
    std::lock_guard<std::mutex> guard(T.lock);
    bool ok = true;
    if (!T.built || std::memcmp(key, T.key, sizeof(key)) != 0) {
        for (hipStream_t u : T.synced)
            if (u != st) ok = ok && hipEventRecord(T.ready, u) == hipSuccess && hipStreamWaitEvent(st, T.ready, 0) == hipSuccess;
        T.synced.clear();
        T.built = false;
        if (ok) {
            k_dp_table_build<<<(2 * pl.half + kBlock) / kBlock, kBlock, 0, st>>>(T.dev, pl.half, std::ldexp(1.0, -pl.k), pl.h,
                                                                                 pl.f, pl.w, pl.r);
            ok = hipGetLastError() == hipSuccess && hipEventRecord(T.ready, st) == hipSuccess;
        }
        if (ok) {
            std::memcpy(T.key, key, sizeof(key));
            T.half = pl.half; T.log2_scale = pl.k; T.built = true;
            T.synced.push_back(st);
        }
    } else if (std::find(T.synced.begin(), T.synced.end(), st) == T.synced.end()) {
        // a reader is never forgotten -- a rebuild has to wait for it --: the 65th stream of one build gets no table
        ok = T.synced.size() < 64 && hipStreamWaitEvent(st, T.ready, 0) == hipSuccess;
        if (ok) T.synced.push_back(st);
    }
    if (!ok) {
        (void)hipGetLastError();
        return false;
    }
    ref.tab = T.dev; ref.scale = (float)std::ldexp(1.0, T.log2_scale);
    ref.lo = (float)(-T.half); ref.hi = (float)(T.half - 1); ref.half = T.half;
    ref.h = (float)pl.h; ref.w = (float)pl.w;                   // make_dp's roundings
    return true;
}

// SDIRT_DP_WEIGHT_TABLE=0 in the environment: every call evaluates the closed form (a test hook: the A/B of
// tests/test_gpu_dp_weight_table.py and of the profiles; read per call, so a test can flip it in one process)
static bool dp_table_enabled()
{
    const char* e = std::getenv("SDIRT_DP_WEIGHT_TABLE");
    return !(e && e[0] == '0' && e[1] == '\0');
}

// sdirt_dp_weight_table_selftest: both forms of the weights on the same abscissae, as k_psf_lr evaluates them
__global__ void __launch_bounds__(kBlock) k_dp_weights_both(DpTableRef t, DevDpParams dp, const float* __restrict__ x_tan, int64_t n,
                                                            float2* __restrict__ lr_table, float2* __restrict__ lr_closed)
{
    const auto div_fmh = UDiv<Lean>::make(dp.fmh);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = x_tan[i];
        float frac, sl, sr;
        const DpTablePair q = dp_table_fetch(t, x, frac);
        dp_table_weights(t, q, frac, x, sl, sr);
        lr_table[i] = make_float2(sl, sr);
        dp_weights_small<Lean>(dp, div_fmh, x, sl, sr);
        lr_closed[i] = make_float2(sl, sr);
    }
}

// forward_integral on a point-major SoA bundle, grids too large for LDS (ks > SDIRT_MAX_KS; the one caller is a
// plot that traces three points): one thread per ray, contributions added to the pre-zeroed [N,ks,ks] grids in HBM
// with global float atomics (the 64 adds of a wave instruction fall into ONE tile).
__global__ void __launch_bounds__(kBlock)
k_forward_integral_hbm(sdirt_rays R, int64_t S, int64_t N, SplatGeom gm, DevDpParams dp,
                       const float* __restrict__ center, float* __restrict__ lg,
                       float* __restrict__ rg)
{
    const int64_t M = S * N;
    const int64_t tile = (int64_t)gm.ks * gm.ks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / S;
        SplatTaps tp;
        if (!splat_taps(gm, R.ox[i], R.oy[i], center[2 * n], center[2 * n + 1], R.ra[i], tp))
            continue;
        const float x_tan = (-R.dx[i]) / R.dz[i];    // monte_carlo.py:48
        float sl, sr;
        if (dp.big) dp_weights_big(dp, x_tan, sl, sr);
        else dp_weights_small(dp, x_tan, sl, sr);
        float* L = lg + n * tile;
        atomicAdd(L + tp.i_tl, tp.w_tl * sl);
        atomicAdd(L + tp.i_tr, tp.w_tr * sl);
        atomicAdd(L + tp.i_bl, tp.w_bl * sl);
        atomicAdd(L + tp.i_br, tp.w_br * sl);
        if (rg && dp.have_r) {
            float* Rr = rg + n * tile;
            atomicAdd(Rr + tp.i_tl, tp.w_tl * sr);
            atomicAdd(Rr + tp.i_tr, tp.w_tr * sr);
            atomicAdd(Rr + tp.i_bl, tp.w_bl * sr);
            atomicAdd(Rr + tp.i_br, tp.w_br * sr);
        }
    }
}

// forward_integral on a point-major SoA bundle with the grids in LDS (monte_carlo.py:9-68 for every ks <=
// SDIRT_MAX_KS).
//
// A workgroup OWNS P consecutive points (one, unless a point has fewer samples than the workgroup has threads)
// and a slice of the spp axis: their L/R tiles live in LDS for the whole kernel (no global atomics, no memset,
// each tile stored once, coalesced) -- or, when the few points of a call are cut along spp (nsplit > 1), added
// once per workgroup to the zeroed output.  Thread t works on sample t % rp of point t / rp (rp = 512 / P): a wave
// reads 64 consecutive samples of one point, 256 contiguous bytes per component (sample-major bundles, the
// reference's tensor order, gave a workgroup 8 to 32 useful bytes of every 128-byte line: 44.8 M L2 requests and
// 352 us for the 16.8 M rays of the staged bench at ks 65, profiles/r04/staged_pmc_sample_major.json).
//
// The tiles are DOUBLES whenever two of them fit (ks <= 99): on gfx950 one ds_add_f32 wave instruction occupies the
// LDS for ~193 cycles whatever its addresses (it is executed lane by lane), ds_add_f64 for 17-30 and ds_add_u64 for
// 8-20 (tools/lds_atomic_bench.hip, profiles/r04/lds_atomic_bench*.txt) -- with eight adds per ray the fp32 form
// IS the kernel's time (350 of 350 us on 8.4 M rays).  A double sum rounded once on the way out is also nearer to
// the reference's sequential fp32 sum's exact value than any fp32 summation order, and takes any weight `ra`.
constexpr int kFiThreads = 512;          // 256 / 512 / 1024 measured on nine batch shapes: 512 is 3-12 % ahead (profiles/r04)
constexpr int kFiDepth = 2;             // passes whose rays are in flight (2, 4, 8 time within 7 %: profiles/r04)
struct FiLaunch {
    int P, logRp;         // points per workgroup; log2(samples per pass and point = kFiThreads / P)
    int ngroups;          // ceil(N / P)
    int nsplit;           // slices of the spp axis
    int64_t chunk;        // samples per slice, a multiple of kFiThreads / P
    int stride;           // accumulators per point in LDS: (ntile * ks * ks) | 1, odd -> the same pixel of different
                          // points never shares a bank
};
template <bool HAVE_R, bool BIG, class ACC, class M>
__global__ void __launch_bounds__(kFiThreads)
k_forward_integral_tiles(sdirt_rays R, int64_t S, int64_t N, SplatGeom gm, DevDpParams dp, FiLaunch fl,
                         const float* __restrict__ center, float* __restrict__ lg, float* __restrict__ rg, int normalize)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fi_lds[];
    __shared__ float fi_red[kFiThreads / 64];
    ACC* __restrict__ fi_tiles = reinterpret_cast<ACC*>(fi_lds);
    const int tile = gm.ks * gm.ks;
    const int g = (int)(blockIdx.x / (uint32_t)fl.nsplit), j = (int)(blockIdx.x - (uint32_t)g * fl.nsplit);
    const int rp = 1 << fl.logRp;
    const int p = threadIdx.x >> fl.logRp, row = threadIdx.x & (rp - 1);
    const int64_t n = (int64_t)g * fl.P + p;
    const bool have_pt = n < N;
    for (int i = threadIdx.x; i < fl.P * fl.stride; i += kFiThreads) fi_tiles[i] = (ACC)0;
    __syncthreads();

    const float cx = have_pt ? center[2 * n] : 0.0f, cy = have_pt ? center[2 * n + 1] : 0.0f;
    ACC* __restrict__ tl_ = fi_tiles + p * fl.stride;
    ACC* __restrict__ trr = tl_ + tile;
    const auto div_dy = UDiv<M>::make(gm.dy_rng), div_dx = UDiv<M>::make(gm.dx_rng);
    const auto div_fmh = UDiv<M>::make(dp.fmh);
    const int64_t s_begin = (int64_t)j * fl.chunk, s_end = min(S, s_begin + fl.chunk);
    const int npass = (int)((s_end - s_begin + rp - 1) >> fl.logRp);     // the same for every thread: no vote, no barrier
    int64_t s = s_begin + row;
    int64_t i = (have_pt ? n : 0) * S + s;
    // The rays of the next kFiDepth passes are in flight while one pass is splatted.  Every thread loads on every
    // pass -- lanes without a ray read element 0 and ignore it -- so that the number of loads in flight is the same on
    // every path: the compiler then waits with a counted s_waitcnt vmcnt for exactly the set it is about to use (a
    // predicated prefetch forces vmcnt(0) right behind its own issue).
    float vox[kFiDepth], voy[kFiDepth], vdx[kFiDepth], vdz[kFiDepth], vra[kFiDepth];
    bool vcur[kFiDepth];
#pragma unroll
    for (int k = 0; k < kFiDepth; ++k) {
        vcur[k] = have_pt && s < s_end;
        const int64_t il = vcur[k] ? i : 0;
        vox[k] = R.ox[il]; voy[k] = R.oy[il]; vdx[k] = R.dx[il]; vdz[k] = R.dz[il]; vra[k] = R.ra[il];
        s += rp; i += rp;
    }
    for (int pass = 0; pass < npass; pass += kFiDepth) {
#pragma unroll
        for (int k = 0; k < kFiDepth; ++k) {
            const float ox = vox[k], oy = voy[k], dx = vdx[k], dz = vdz[k], ra = vra[k];
            const bool cur = vcur[k];
            vcur[k] = have_pt && s < s_end;
            const int64_t il = vcur[k] ? i : 0;
            vox[k] = R.ox[il]; voy[k] = R.oy[il]; vdx[k] = R.dx[il]; vdz[k] = R.dz[il]; vra[k] = R.ra[il];
            s += rp; i += rp;
            SplatTaps tp;
            if (cur && splat_taps(gm, div_dy, div_dx, ox, oy, cx, cy, ra, tp)) {
                const float x_tan = (-dx) / dz;              // monte_carlo.py:48
                float sl, sr;
                if (BIG) dp_weights_big(dp, x_tan, sl, sr);
                else dp_weights_small<M>(dp, div_fmh, x_tan, sl, sr);
                atomicAdd(&tl_[tp.i_tl], (ACC)(tp.w_tl * sl));
                atomicAdd(&tl_[tp.i_tr], (ACC)(tp.w_tr * sl));
                atomicAdd(&tl_[tp.i_bl], (ACC)(tp.w_bl * sl));
                atomicAdd(&tl_[tp.i_br], (ACC)(tp.w_br * sl));
                if (HAVE_R) {
                    atomicAdd(&trr[tp.i_tl], (ACC)(tp.w_tl * sr));
                    atomicAdd(&trr[tp.i_tr], (ACC)(tp.w_tr * sr));
                    atomicAdd(&trr[tp.i_bl], (ACC)(tp.w_bl * sr));
                    atomicAdd(&trr[tp.i_br], (ACC)(tp.w_br * sr));
                }
            }
        }
    }
    __syncthreads();
    // the P tiles of this workgroup are P * ks * ks consecutive floats of the [N, ks, ks] output
    const int np = (int)min((int64_t)fl.P, N - (int64_t)g * fl.P);
    for (int pp = 0; pp < np; ++pp) {
        const ACC* __restrict__ src = fi_tiles + pp * fl.stride;
        float* __restrict__ Lg = lg + ((int64_t)g * fl.P + pp) * tile;
        float* __restrict__ Rg = HAVE_R ? rg + ((int64_t)g * fl.P + pp) * tile : nullptr;
        if (fl.nsplit == 1 && normalize) {
            // optics.py:983-987 on the way out (SDIRT_PSF_NORMALIZE): psf / (max + 1e-6) of the float grids, the same
            // values and the same division k_psf_normalize would read back and perform
            float ml = -INFINITY, mr = -INFINITY;
            for (int e = threadIdx.x; e < tile; e += kFiThreads) {
                ml = fmaxf(ml, (float)src[e]);
                if (HAVE_R) mr = fmaxf(mr, (float)src[tile + e]);
            }
            const float dl = block_max(ml, fi_red) + 1e-6f;
            const float dr = HAVE_R ? block_max(mr, fi_red) + 1e-6f : 1.0f;
            for (int e = threadIdx.x; e < tile; e += kFiThreads) {
                Lg[e] = (float)src[e] / dl;
                if (HAVE_R) Rg[e] = (float)src[tile + e] / dr;
            }
        } else if (fl.nsplit == 1) {
            for (int e = threadIdx.x; e < tile; e += kFiThreads) {
                Lg[e] = (float)src[e];
                if (HAVE_R) Rg[e] = (float)src[tile + e];
            }
        } else {
            for (int e = threadIdx.x; e < tile; e += kFiThreads) {
                const float a = (float)src[e];
                if (a != 0.0f) atomicAdd(&Lg[e], a);
                if (HAVE_R) {
                    const float c = (float)src[tile + e];
                    if (c != 0.0f) atomicAdd(&Rg[e], c);
                }
            }
        }
    }
}

// optics.py:983-987: one workgroup per point.  LDS_TILE: the tile is read from HBM once, into LDS (grids up to
// ks 110: 48 KB), its maximum taken there and the quotients written back -- one read and one write per pixel; larger grids
// are read twice (the second pass mostly out of L2).
// `stride`: floats between the grids of consecutive points (tile, or 2 * tile for one half of an interleaved [N, 2, ks, ks] array).
template <bool LDS_TILE>
__global__ void __launch_bounds__(kBlock) k_psf_normalize(float* __restrict__ psf, int tile, int64_t stride)
{
    extern __shared__ __attribute__((aligned(16))) float nz_tile[];
    __shared__ float red[kBlock / 64];
    float* g = psf + (int64_t)blockIdx.x * stride;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < tile; i += blockDim.x) {
        const float v = g[i];
        if (LDS_TILE) nz_tile[i] = v;
        mx = fmaxf(mx, v);
    }
    mx = block_max(mx, red);
    const float den = mx + 1e-6f;
    for (int i = threadIdx.x; i < tile; i += blockDim.x) g[i] = (LDS_TILE ? nz_tile[i] : g[i]) / den;
}

// ---------------------------------------------------------------------------
// fused kernels
// ---------------------------------------------------------------------------

// The END of a launch with one workgroup per point.  The SIMDs serve the OLDEST wave first, so of the four workgroups that
// share a CU the oldest runs ahead and the youngest is left to finish alone, at 2 waves per SIMD (0.6-0.8 of the 8-wave
// rate of these kernels) -- in the middle of a launch a younger workgroup takes the freed slot, at its end nobody does:
// 0.13 ms per launch of k_psf_lr whatever its length (profiles/r05/launch_fixed_cost.txt).  Workgroups of the LAST
// generation (the last 4 x CUs blocks: `prio_from`) therefore set their waves' issue priority -- s_setprio, which ranks
// above age -- by the passes they still have to run, one level per kPrioStep passes: whoever is behind is served first
// and the workgroups of a CU finish together.  A scheduling hint only: the results are the same bit for bit.
// Measured (profiles/r06/prio_ab_levels*.txt, same box, warm): config 2 cut to 1024 / 2048 / 4096 / 16384 points
// 0.670 / 1.233 / 2.348 / 9.02 ms -> 0.596 / 1.164 / 2.275 / 8.93; one level per 1 or 3 passes, per quarter of the work, a
// constant priority for the older generations, two generations, every workgroup: all behind.  Cutting the last
// generation into smaller work units on top of it (slices of spp whose partial tiles the last slice to arrive adds up:
// commit acacd51, profiles/r06/tail_ab_*.txt) never added anything: what such a slice saves at the end of the launch it
// pays at its own start and end.
constexpr int kPrioStep = 2;
__device__ __forceinline__ void prio_by_work_left(int passes_left)
{
    const int q = (passes_left - 1) / kPrioStep;        // 3+: seven or more passes to go ... 0: the last two
    if (q >= 3) __builtin_amdgcn_s_setprio(3);
    else if (q == 2) __builtin_amdgcn_s_setprio(2);
    else if (q == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

// What a ray starts from and ends at, the same for every ray of a workgroup: wave-uniform but only ever vector
// operands, so the kernels that have the VGPRs for it keep them there (in_vgpr).
struct RayEnds {
    float px, py, pzo;       // the object point
    float pz, zs;            // the pupil plane's distance from it, the sensor plane
};

// THE sample loop of this file: lane t traces samples s0, s0 + THREADS, ... < s_end of (xs, ys) from the point through
// `lens` to the sensor plane and hands each ray to per_ray.  PIN: this lane's sample addresses and the end of its loop
// per lane, in VGPRs (in_vgpr_if), else indexed from the arrays.  PRIO: the issue priority counts DOWN the passes
// that are left (prio_by_work_left; a workgroup that is not of the last generation starts at kNoPrio, so far below zero
// that it never gets there), compiled out otherwise.
template <class HotMath, int THREADS, bool PIN, bool PRIO, class Samples, class PerRay>
__device__ __forceinline__ void for_each_traced_ray(const DevSurface* __restrict__ lens, int K, const void* trips,
                                                    const RayEnds& e, Samples xs, Samples ys, int s0, int s_end,
                                                    int passes_left, uint32_t* lds_mask, PerRay per_ray)
{
    GlobalF xp = in_vgpr_if<PIN>((GlobalF)(xs + s0));
    GlobalF yp = in_vgpr_if<PIN>((GlobalF)(ys + s0));
    const int end = in_vgpr_if<PIN>(s_end);
    for (int s = s0, left = passes_left; s < end; s += THREADS, --left) {
        if constexpr (PRIO) { if (left > 0) prio_by_work_left(left); }
        Ray r = make_ray<HotMath>(e.px, e.py, e.pzo, PIN ? *xp : xs[s], PIN ? *yp : ys[s], e.pz);
        if constexpr (PIN) { xp += THREADS; yp += THREADS; }
        trace_ray<true, HotMath, true, true, true, /*WAVE*/ true>(lens, 0, K, trips, r, lds_mask);
        propagate_to<HotMath>(r, e.zs);
        per_ray(r);
    }
}
constexpr int kNoPrio = INT32_MIN / 2;

// A lane's share of the chief-ray centroid: fp64 sums of (x * ra, y * ra, ra) and whether any of its rays arrived.
struct ChiefSums {
    double sx = 0.0, sy = 0.0, sr = 0.0;
    int any = 0;
    __device__ __forceinline__ void add(const Ray& r)
    {
        sx += (double)(r.ox * r.ra);
        sy += (double)(r.oy * r.ra);
        sr += (double)r.ra;
        any |= (r.ra == 1.0f);
    }
};
// ... over the lane's samples of for_each_traced_ray; `extra` sees every ray after it was added
template <class HotMath, int THREADS, bool PIN, bool PRIO, class Samples, class Extra>
__device__ __forceinline__ ChiefSums chief_ray_sums(const DevSurface* __restrict__ lens, int K, const void* trips,
                                                    const RayEnds& e, Samples xs, Samples ys, int s0, int s_end,
                                                    int passes_left, uint32_t* lds_mask, Extra extra)
{
    ChiefSums a;
    for_each_traced_ray<HotMath, THREADS, PIN, PRIO>(lens, K, trips, e, xs, ys, s0, s_end, passes_left, lds_mask, [&](const Ray& r) {
        a.add(r);
        extra(r);
    });
    return a;
}

// The start of a chief kernel's workgroup: the masks and the flag cleared, the point and the planes in VGPRs.
__device__ __forceinline__ RayEnds chief_prologue(uint32_t* lds_mask, int* red_any, const float* __restrict__ po, int n,
                                                  float pz, float zs)
{
    if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
    if (threadIdx.x == 0) *red_any = 0;
    __syncthreads();
    RayEnds e;
    e.px = in_vgpr(po[3 * n]); e.py = in_vgpr(po[3 * n + 1]); e.pzo = in_vgpr(po[3 * n + 2]);
    e.pz = in_vgpr(pz); e.zs = in_vgpr(zs);
    return e;
}

// psf_center: one workgroup per point, Sc rays, fp64 partial sums reduced in a fixed order (deterministic).
// SLOPE (sdirt_chief_center_slope) also returns how the centre moves with the sensor plane: the sensor-plane point of a
// ray is o = o' + d (zs - o'.z) / d.z, so with c = -sum(ra o.xy) / (sum(ra) + 1e-9)
//   dc/dzs = -sum(ra d.xy / d.z) / (sum(ra) + 1e-9).
// The slope terms are float64 from the fp32 direction after the last surface, summed per lane and then over the
// workgroup by reduce_centroid, through the same LDS block once the centroid's totals have been read.  The centre is
// the same in both forms because both are chief_ray_sums, reduce_centroid and centre_from_sums; everything of the slope
// is under `if constexpr (SLOPE)`, so the plain form carries none of it.  Work-left priorities in the plain form only:
// the slope pass runs once per gradient call, beside a staged trace.
template <class HotMath, bool SLOPE>
__global__ void __launch_bounds__(kFused, 8)
k_chief_center(TripTable trips /* kernarg offset 0 */, const DevSurface* __restrict__ lens, int K,
               const float* __restrict__ po, const float* __restrict__ xc,
               const float* __restrict__ yc, int Sc, float pz, float zs,
               float* __restrict__ center, double* __restrict__ slope, int32_t* __restrict__ any_valid,
               uint32_t* __restrict__ conv_mask, int prio_from)
{
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    __shared__ double red[3][kFused];
    __shared__ int red_any;
    const int n = blockIdx.x;
    const bool by_work_left = (int)blockIdx.x >= prio_from;
    const int passes = (Sc + kFused - 1) / kFused;
    const RayEnds e = chief_prologue(lds_mask, &red_any, po, n, pz, zs);
    double tx = 0.0, ty = 0.0;
    const ChiefSums a = chief_ray_sums<HotMath, kFused, true, !SLOPE>(
        lens, K, kernarg_at(0), e, xc, yc, (int)threadIdx.x, Sc, by_work_left ? passes : kNoPrio, lds_mask, [&](const Ray& r) {
            if constexpr (SLOPE) {
                if (r.ra != 0.0f) {                       // a dead ray's direction is whatever the trace left
                    const double z = (double)r.dz;
                    tx += (double)r.ra * ((double)r.dx / z);
                    ty += (double)r.ra * ((double)r.dy / z);
                }
            }
        });
    if constexpr (!SLOPE) __builtin_amdgcn_s_setprio(0);
    red[0][threadIdx.x] = a.sx; red[1][threadIdx.x] = a.sy; red[2][threadIdx.x] = a.sr;
    if (a.any) red_any = 1;
    reduce_centroid<kFused>(&red[0][0]);
    const double sum_ra = red[2][0];
    if (threadIdx.x == 0) {
        const float2 c = centre_from_sums(red[0][0], red[1][0], red[2][0]);
        center[2 * n] = c.x;
        center[2 * n + 1] = c.y;
        if (any_valid && red_any) atomicOr(any_valid, 1);
    }
    if constexpr (SLOPE) {
        __syncthreads();                          // everyone has read the centroid's totals: the block is free again
        red[0][threadIdx.x] = tx; red[1][threadIdx.x] = ty; red[2][threadIdx.x] = 0.0;
        reduce_centroid<kFused>(&red[0][0]);
        if (threadIdx.x == 0) {
            const double den = sum_ra + 1e-9;
            slope[2 * n] = -(red[0][0] / den);
            slope[2 * n + 1] = -(red[1][0] / den);
        }
    }
    if (conv_mask && (int)threadIdx.x < K && lds_mask[threadIdx.x])
        atomicOr(&conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// speculate -> verify ON THE DEVICE -> re-render once (sdirt_psf_lr_verified)
// ---------------------------------------------------------------------------
// Control block of a verified call, uint32 words in device memory (zeroed by the caller):
// what the host needs to accept the result -- or to go on correcting -- in ONE readback.
constexpr int kCtlStatus = SDIRT_CTL_STATUS, kCtlAnyValid = SDIRT_CTL_ANY_VALID,
              kCtlTrips2P = SDIRT_CTL_TRIPS2, kCtlTrips2C = SDIRT_CTL_TRIPS2 + 16,
              kCtlMask1P = SDIRT_CTL_MASKS, kCtlMask1C = SDIRT_CTL_MASKS + 64,
              kCtlMask2P = SDIRT_CTL_MASKS + 128, kCtlMask2C = SDIRT_CTL_MASKS + 192;
static_assert(kCtlMask2C + 64 == SDIRT_CTL_WORDS, "control block layout");

// Arguments of the split path (several workgroups per point) of a verified call.
struct SplitArgs {
    const uint32_t* gate;        // round 2: the control block; the kernel returns at once when its
                                 // status word says that round 1 was already right
    const uint32_t* trips_dev;   // round 2: the corrected trip table (TripTable layout) in device memory
    const double* part;          // chief-ray partial sums [N][nslice][3] (sx, sy, sr), or nullptr
    int nslice;
};

// The chief-ray pass of a point cut into `nslice` workgroups (N = 64 points alone leave three
// quarters of the chip idle and every lane with four rays in a row): each writes its fp64 partial
// sums; the consumers add them in slice order (a fixed order: deterministic).  Also clears the
// output grids the primary pass will add to (global float atomics).
template <class HotMath>
__global__ void __launch_bounds__(kFused, 8)
k_chief_slices(TripTable trips /* kernarg offset 0 */, SplitArgs sa, const DevSurface* __restrict__ lens, int K,
               const float* __restrict__ po, const float* __restrict__ xc, const float* __restrict__ yc,
               int Sc, int chunk, float pz, float zs, double* __restrict__ part, uint32_t* __restrict__ any_valid,
               uint32_t* __restrict__ conv_mask, float* __restrict__ zero_a, float* __restrict__ zero_b,
               int64_t zero_n)
{
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    __shared__ double red[3][kFused];
    __shared__ int red_any;
    if (sa.gate && sa.gate[kCtlStatus] == 0u) return;              // wave-uniform
    const void* trip_words = sa.trips_dev ? (const void*)sa.trips_dev : kernarg_at(0);
    const int n = blockIdx.x / sa.nslice, j = blockIdx.x - n * sa.nslice;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < zero_n; i += (int64_t)gridDim.x * blockDim.x) {
        zero_a[i] = 0.0f;
        if (zero_b) zero_b[i] = 0.0f;
    }
    const RayEnds e = chief_prologue(lds_mask, &red_any, po, n, pz, zs);
    const ChiefSums a = chief_ray_sums<HotMath, kFused, true, false>(
        lens, K, trip_words, e, xc, yc, j * chunk + (int)threadIdx.x, min(Sc, (j + 1) * chunk), kNoPrio, lds_mask, [](const Ray&) {});
    red[0][threadIdx.x] = a.sx; red[1][threadIdx.x] = a.sy; red[2][threadIdx.x] = a.sr;
    if (a.any) red_any = 1;
    reduce_centroid<kFused>(&red[0][0]);
    if (threadIdx.x == 0) {
        double* o = part + (int64_t)blockIdx.x * 3;
        o[0] = red[0][0]; o[1] = red[1][0]; o[2] = red[2][0];
        if (red_any) atomicOr(any_valid, 1u);
    }
    if ((int)threadIdx.x < K && lds_mask[threadIdx.x]) atomicOr(&conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

// sdirt_amd/newton.py: verify() on the device.  `t` ran, `mask` is what it reported; writes the
// table the next round should run (t itself when it was exactly the reference's) and says whether
// t was right.  One thread; K <= 64.
__device__ bool verify_trips(const TripTable& t, const uint32_t* __restrict__ mask,
                             const DevSurface* __restrict__ lens, int K, uint32_t* __restrict__ out_words)
{
    uint32_t nw[SDIRT_MAX_SURFACES / 4];
    for (int i = 0; i < SDIRT_MAX_SURFACES / 4; ++i) nw[i] = t.w[i];
    bool failed = false;
    for (int k = 0; k < K; ++k) {
        const int sh = (k & 3) * 8;
        const int T = (int)(int8_t)(t.w[k >> 2] >> sh);
        int nv;
        if ((lens[k].h.flags & 3u) == 0u) {
            nv = 0;                                            // planes: no Newton solve
        } else {
            int j = 0;                                         // first clear bit among 1..T
            const uint32_t m = mask[k];
            for (int b = 1; b <= T; ++b)
                if (!((m >> b) & 1u)) { j = b; break; }
            if (!failed) {
                if (T >= 1 && (j == T || (j == 0 && T == SDIRT_NEWTON_MAXITER))) continue;
                failed = true;
            }
            nv = j ? j : min(max(T, 0) + 1, SDIRT_NEWTON_MAXITER);
        }
        nw[k >> 2] = (nw[k >> 2] & ~(0xffu << sh)) | ((uint32_t)(uint8_t)(int8_t)nv << sh);
    }
    for (int i = 0; i < SDIRT_MAX_SURFACES / 4; ++i) out_words[i] = failed ? nw[i] : t.w[i];
    return !failed;
}

// sdirt_psf_call's prologue as ONE launch: both pupil mappings of a psf call (u = [theta | r2 | theta_c | r2_c] ->
// xy = [x2 | y2 | xc | yc], sdirt_pupil_samples twice) and, on request, the clearing of the control block.
__global__ void __launch_bounds__(kBlock) k_pupil_pair(const float* __restrict__ u, int S, int Sc, float pr2, float pr2c,
                                                       float* __restrict__ xy, uint32_t* __restrict__ zero, int nzero)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nzero) zero[i] = 0u;
    if (i < S) pupil_point(u[i], u[S + i], pr2, xy[i], xy[S + i]);
    else if (i < S + Sc) {
        const int c = i - S;
        pupil_point(u[2 * S + c], u[2 * S + Sc + c], pr2c, xy[2 * S + c], xy[2 * S + Sc + c]);
    }
}

// The trip verdict of round 1: tp and tc ran and left their masks in the control block; the tables round 2 should run
// go beside them, and status 0 when both were the reference's, else 1 | 2 (tp wrong) | 4 (tc wrong).  One thread.
__device__ __forceinline__ void verify_round(uint32_t* ctl, const DevSurface* lens, int K, const TripTable& tp,
                                             const TripTable& tc)
{
    const bool okp = verify_trips(tp, ctl + kCtlMask1P, lens, K, ctl + kCtlTrips2P);
    const bool okc = verify_trips(tc, ctl + kCtlMask1C, lens, K, ctl + kCtlTrips2C);
    ctl[kCtlStatus] = (okp && okc) ? 0u : (1u | (okp ? 0u : 2u) | (okc ? 0u : 4u));
}

// The trip rule on the device for a call with one workgroup per point (sdirt_psf_call): round 1's masks stand in the
// control block; status and the tables a correction would run go beside them.  One thread.
__global__ void k_ctl_verify(uint32_t* __restrict__ ctl, const DevSurface* __restrict__ lens, int K, TripTable tp, TripTable tc)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    verify_round(ctl, lens, K, tp, tc);
}

// Round 1's masks and the any-valid flag of a control block as 0 / 1 lanes -- [primary | chief][surface][bit 0..10],
// then the flag -- so that ranks can OR them with an all-reduce(MAX) (RCCL has no bitwise OR), and back.
constexpr int kLaneBits = SDIRT_NEWTON_MAXITER + 1;
constexpr int kMaskLanes = 2 * SDIRT_MAX_SURFACES * kLaneBits;       // then: any-valid, uniform sum, its complement
static_assert(kMaskLanes + 3 == SDIRT_CTL_LANES, "lane layout");
__global__ void __launch_bounds__(kBlock) k_ctl_to_lanes(const uint32_t* __restrict__ ctl, uint32_t tag, int32_t* __restrict__ lanes)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= SDIRT_CTL_LANES) return;
    if (i == kMaskLanes) { lanes[i] = ctl[kCtlAnyValid] != 0u; return; }
    // the caller's tag and its complement: after a MAX over ranks the two still add up to 0x3fffffff iff all ranks agreed
    if (i > kMaskLanes) { lanes[i] = (int32_t)(i == kMaskLanes + 1 ? (tag & 0x3fffffffu) : 0x3fffffffu - (tag & 0x3fffffffu)); return; }
    const int word = i / kLaneBits, bit = i - word * kLaneBits;      // word: 0..63 primary, 64..127 chief
    lanes[i] = (int32_t)((ctl[kCtlMask1P + word] >> bit) & 1u);
}
__global__ void __launch_bounds__(2 * SDIRT_MAX_SURFACES) k_ctl_from_lanes(const int32_t* __restrict__ lanes, uint32_t* __restrict__ ctl,
                                                                         const DevSurface* __restrict__ lens, int K, TripTable tp, TripTable tc)
{
    const int word = threadIdx.x;                                    // 128 threads, one mask word each
    uint32_t m = 0u;
    for (int b = 0; b < kLaneBits; ++b) m |= (lanes[word * kLaneBits + b] != 0 ? 1u : 0u) << b;
    ctl[kCtlMask1P + word] = m;
    if (word == 0) ctl[kCtlAnyValid] = lanes[kMaskLanes] != 0 ? 1u : 0u;
    if (word == 1 || word == 2) ctl[SDIRT_CTL_TAG + word - 1] = (uint32_t)lanes[kMaskLanes + word];
    __syncthreads();
    if (word == 0 && lens) verify_round(ctl, lens, K, tp, tc);
}

// Last kernel of a round of the split path: max-normalise L (blockIdx.y 0) and R (1), and -- round 1
// -- check both trip tables against the masks the round produced: status 0 = the reference's tables,
// nothing more to do; else bit 0 set (bit 1: primary table wrong, bit 2: chief-ray table wrong) and
// the corrected tables stand in the control block for round 2, which is already enqueued.
struct FinishArgs {
    const uint32_t* gate;      // round 2: skip unless status != 0
    uint32_t* ctl;             // round 1: verify into this block (nullptr: no verification)
    const DevSurface* lens;    // surface kinds (the same in every wavelength's table)
    int K;
    TripTable tp, tc;          // the tables round 1 ran
};
__global__ void __launch_bounds__(kBlock) k_psf_finish(float* __restrict__ l, float* __restrict__ r, int tile,
                                                       int64_t pstride, int normalize, FinishArgs fa)
{
    __shared__ float red[kBlock / 64];
    if (fa.gate && fa.gate[kCtlStatus] == 0u) return;
    float* g = (blockIdx.y == 0 ? l : r) + (int64_t)blockIdx.x * pstride;
    if (normalize) {
        float mx = -INFINITY;
        for (int i = threadIdx.x; i < tile; i += blockDim.x) mx = fmaxf(mx, g[i]);
        mx = block_max(mx, red);
        const float den = mx + 1e-6f;
        for (int i = threadIdx.x; i < tile; i += blockDim.x) g[i] = g[i] / den;
    }
    if (fa.ctl && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) verify_round(fa.ctl, fa.lens, fa.K, fa.tp, fa.tc);
}

// psf_diff fused: sample -> trace -> propagate -> window -> DP weights -> LDS
// splat -> (max-normalise) -> store.  gridDim.x = N * nsplit; the workgroup
// (n, j) handles samples [j*chunk, (j+1)*chunk) of point n.
//   nsplit == 1 : the tile is complete in LDS -> normalise (flag) and store.
//   nsplit  > 1 : tiles are added to the pre-zeroed output with global float
//                 atomics; the caller normalises afterwards.
// Arguments of the optional in-kernel chief-ray pass (CENTER instantiations, nsplit == 1): the
// workgroup first traces the Sc shrunk-pupil samples of its point through the GREEN lens table
// (optics.py:900), reduces the centroid exactly like k_chief_center, and only then splats.
struct CenterArgs {
    const DevSurface* lens_c;
    const float* xc;
    const float* yc;
    int Sc;
    float* center_out;       // [N,2]
    int32_t* any_valid;
    uint32_t* conv_mask_c;
};

// __launch_bounds__(512, 8): four workgroups per CU = 8 waves per SIMD (<= 80 SGPRs, <= 64 VGPRs).
// The big-radius microlens branch (corner-clipped areas, monte_carlo.py:242-372) needs ~90 VGPRs:
// capped at 64 it would spill 60 of them to scratch, so it runs at 4 waves per SIMD instead.
// `sb`, `lb`, `prim` and `trips_c` MUST stay the first four parameters: the kernel reads them as 64-byte blocks at fixed
// offsets of its kernel-argument segment (0, 64, 128, 128 + 128 W: SplatBlock, LoopBlock, PrimarySet, TripSet) and never
// through the parameters themselves.
// blockIdx.y = wavelength slot w of a multi-wavelength launch (psf_rgb: gridDim.y = 3, one lens
// table, pupil sample set, trip table and mask row per slot; a plain call has gridDim.y = 1): the
// output is [N, gridDim.y, ks, ks], the reference's psf_rgb layout (optics.py:1015).
struct LensSet {
    const DevSurface* p[SDIRT_MAX_WAVELENGTHS];
};
struct TripSet {
    TripTable t[SDIRT_MAX_WAVELENGTHS];
};
// The primary trip table of each wavelength slot with a copy of the splat block right behind it: the address of its
// trip table is the one pointer into the argument segment a primary ray holds while it is traced, and the splat's
// constants are found 64 bytes behind it -- no second pointer to keep (or park) for the end of the ray.
struct PrimarySet {
    struct Slot {
        TripTable t;
        SplatBlock sb;
    } s[SDIRT_MAX_WAVELENGTHS];
};
static_assert(sizeof(PrimarySet::Slot) == 128 && offsetof(PrimarySet::Slot, sb) == 64, "layout");
// ACC = the accumulator type of the LDS tiles.  float: ds_add_f32, which gfx950 executes lane by lane (~193 cycles
// of the CU's LDS per wave instruction whatever the addresses, profiles/r04/lds_atomic_bench.txt); double:
// ds_add_f64 (17-33 cycles), the sum rounded to fp32 once on the way out like k_forward_integral_tiles -- chosen by
// plan_psf whenever the double tiles still leave room for four workgroups per CU (L + R: ks <= 49).
// THREADS = 1024 (SDIRT_PSF_DETERMINISTIC on grids of 50 to 70 pixels): double tiles in workgroups of 16 waves, two per
// CU -- the same 8 waves per SIMD; a workgroup waits at its barriers for the slowest of 16 waves: +0.5 % (profiles/r05/ab_tiles.txt).
// TAB (Lean, r <= 0.5 only): the dual-pixel weights come from the sensor's table (dp_table_for) -- words 7..14 of
// the splat block are its DpTableRef -- instead of dp_weights_small.
template <bool HAVE_R, bool BIG, class HotMath, bool CENTER, class ACC, int THREADS = kFused, bool TAB = false>
__global__ void __launch_bounds__(THREADS, BIG ? 4 : 8)
k_psf_lr(SplatBlock sb /* kernarg offset 0 */, LoopBlock lb /* 64 */, PrimarySet prim /* 128 */, TripSet trips_c /* 128 + 128 W */,
         LensSet lens_set, float tr, float tl, const float* __restrict__ center, uint32_t flags, float* __restrict__ lout,
         float* __restrict__ rout, uint32_t* __restrict__ conv_mask, CenterArgs ca, SplitArgs sa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tiles_raw[];
    ACC* __restrict__ tiles = reinterpret_cast<ACC*>(tiles_raw);    // [L | R] ks*ks each
    if (!CENTER && sa.gate && sa.gate[kCtlStatus] == 0u) return;    // round 2 of a verified call, nothing to redo
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    __shared__ float red[THREADS / 64];
    __shared__ float c_sh[2];
    constexpr bool kPin = HotMath::kFused && !BIG;
    const auto pin = [](auto v) { return in_vgpr_if<kPin>(v); };
    constexpr int kLoopAt = 64, kTripsAt = 128, kTripsCAt = 128 + 128 * SDIRT_MAX_WAVELENGTHS;
    // the loop block (LoopBlock): read once, here; the launch is THREADS wide, so the loops step by the constant
    const u32x16 lq = sload_block(kernarg_at(kLoopAt));
    const auto lw = [&](int i) { return in_sgpr(lq[i]); };         // a word of it, on its own: the sixteen are dead behind this
    const auto lptr = [&](int i) { return reinterpret_cast<GlobalF>((uint64_t)lw(i) | ((uint64_t)lw(i + 1) << 32)); };
    GlobalF x2 = lptr(0);
    GlobalF y2 = lptr(2);
    GlobalF po = lptr(4);
    const int S = (int)lw(6), chunk = (int)lw(7), nsplit = (int)lw(8), K = (int)lw(9);
    const float pz = pin(__uint_as_float(lw(10))), zs_s = __uint_as_float(lw(11));
    const int ks = (int)lw(12), prio_from = (int)lw(14);
    __builtin_assume(K >= 1);                     // sdirt_lens_create takes no lens without a surface
    const int tile = ks * ks;
    ACC* tl_ = tiles;
    const int n = blockIdx.x / nsplit;
    const int j = blockIdx.x - n * nsplit;
    const int w = blockIdx.y;
    const int N = gridDim.x / nsplit;
    // the last generation of the launch issues by the passes a workgroup still has to run (prio_by_work_left)
    const bool by_work_left = (int)(blockIdx.y * gridDim.x + blockIdx.x) >= prio_from;
    const int passes_p = (min(S, (j + 1) * chunk) - j * chunk + THREADS - 1) / THREADS;
    const int passes_c = CENTER ? (ca.Sc + THREADS - 1) / THREADS : 0;
    const DevSurface* __restrict__ lens = lens_set.p[w];
    x2 += (int64_t)w * S; y2 += (int64_t)w * S;
    if (conv_mask) conv_mask += w * SDIRT_MAX_SURFACES;
    if (CENTER) {
        ca.xc += (int64_t)w * ca.Sc; ca.yc += (int64_t)w * ca.Sc;
        ca.center_out += (int64_t)w * N * 2;
        if (ca.any_valid) ca.any_valid += w;
        if (ca.conv_mask_c) ca.conv_mask_c += w * SDIRT_MAX_SURFACES;
    } else if (center) {
        center += (int64_t)w * N * 2;
    }
    // the point, the pupil plane's distance from it and the sensor plane: vector operands of every ray
    const RayEnds e = {pin(po[3 * n]), pin(po[3 * n + 1]), pin(po[3 * n + 2]), pz, pin(zs_s)};

    if (CENTER) {
        // ---- chief-ray centre of this point: k_chief_center's sums (ChiefSums::add), reduction (reduce_centroid) and
        // finish (centre_from_sums); the fp64 scratch aliases the not-yet-used tile memory.  The loop is for_each_traced_ray's
        // text once more: called from here, the three strict-IEEE L + R instantiations (BIG = false; at their VGPR budget,
        // the point reloaded from scratch per ray) get another register assignment, one v_mov more per chief ray.
        double* redd = reinterpret_cast<double*>(tiles_raw);         // [3][THREADS]
        if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
        if (threadIdx.x == 0) c_sh[0] = 0.0f;
        __syncthreads();
        ChiefSums a;
        GlobalF xcp = pin((GlobalF)(ca.xc + threadIdx.x));
        GlobalF ycp = pin((GlobalF)(ca.yc + threadIdx.x));
        const int sc_end = pin(ca.Sc);
        int left = by_work_left ? passes_c + passes_p : kNoPrio;             // the primary passes count as well
        for (int s = threadIdx.x; s < sc_end; s += THREADS, --left) {
            if (left > 0) prio_by_work_left(left);
            Ray r = make_ray<HotMath>(e.px, e.py, e.pzo, kPin ? *xcp : ca.xc[s], kPin ? *ycp : ca.yc[s], e.pz);
            if constexpr (kPin) { xcp += THREADS; ycp += THREADS; }
            // (the masks of a call that asks for none are gathered all the same and dropped below: one flag less to keep)
            trace_ray<true, HotMath, true, true, true, /*WAVE*/ true>(ca.lens_c, 0, K, kernarg_at(kTripsCAt + 64 * w), r,
                                                                      lds_mask);
            propagate_to<HotMath>(r, e.zs);
            a.add(r);
        }
        redd[threadIdx.x] = a.sx; redd[THREADS + threadIdx.x] = a.sy; redd[2 * THREADS + threadIdx.x] = a.sr;
        if (a.any) c_sh[0] = 1.0f;                                   // benign race: all write 1
        reduce_centroid<THREADS>(redd);
        if (ca.conv_mask_c && (int)threadIdx.x < K && lds_mask[threadIdx.x])
            atomicOr(&ca.conv_mask_c[threadIdx.x], lds_mask[threadIdx.x]);
        const float any_f = c_sh[0];
        const float2 cc = centre_from_sums(redd[0], redd[THREADS], redd[2 * THREADS]);
        __syncthreads();                                             // everyone has read redd / c_sh
        if (threadIdx.x == 0) {
            ca.center_out[2 * n] = cc.x; ca.center_out[2 * n + 1] = cc.y;
            c_sh[0] = cc.x; c_sh[1] = cc.y;
            if (ca.any_valid && any_f != 0.0f) atomicOr(ca.any_valid, 1);
        }
    }

    const bool from_parts = !CENTER && sa.part != nullptr;
    if (from_parts && threadIdx.x == 0) {
        // the chief-ray centre from the slices' partial sums, added in slice order (k_chief_slices)
        double sx = 0.0, sy = 0.0, sr = 0.0;
        for (int q = 0; q < sa.nslice; ++q) {
            const double* pq = sa.part + ((int64_t)n * sa.nslice + q) * 3;
            sx += pq[0]; sy += pq[1]; sr += pq[2];
        }
        const float2 cc = centre_from_sums(sx, sy, sr);
        c_sh[0] = cc.x;
        c_sh[1] = cc.y;
        if (j == 0) { ca.center_out[2 * n] = c_sh[0]; ca.center_out[2 * n + 1] = c_sh[1]; }
    }
    for (int i = threadIdx.x; i < (HAVE_R ? 2 : 1) * tile; i += blockDim.x) tiles[i] = (ACC)0;
    if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
    __syncthreads();

    const float cx = pin((CENTER || from_parts) ? c_sh[0] : center[2 * n]);
    const float cy = pin((CENTER || from_parts) ? c_sh[1] : center[2 * n + 1]);
    const int s_end = min(S, (j + 1) * chunk);
    const void* kernarg = kernarg_at(0);
    // the reciprocals of the window's extent, the same for every ray of the launch: once per workgroup (Lean; the
    // quotient of a ray stays Lean::div_y with this y -- the same bits; Ieee divides by the extent itself)
    float rcp_dy = 0.0f, rcp_dx = 0.0f;
    if constexpr (HotMath::kFused) {
        const u32x16 q = sload_block(kernarg);
        rcp_dy = pin(Lean::recip(__uint_as_float(q[4])));
        rcp_dx = pin(Lean::recip(__uint_as_float(q[3])));
    }
    // the primary trip table: in the argument segment, found from the segment's own address like the splat block, or
    // (round 2 of a verified call) the corrected one in device memory
    const bool trips_in_mem = !CENTER && sa.trips_dev;
    const void* primary_trips = trips_in_mem ? (const void*)sa.trips_dev : kernarg_at(kTripsAt + 128 * w);
    auto splat = [&](float sx, float sy, float dx, float dz, float ra) {
        // the splat constants: one 64-byte scalar load per ray, dead again after the splat
        // (behind the trip table where that is known to stand in the argument segment, else the copy at offset 0)
        const u32x16 q = CENTER ? sload_block<64>(primary_trips) : sload_block(kernarg);
        const auto F = [&](int i) { return __uint_as_float(q[i]); };
        SplatGeom gm;
        gm.lim = F(0); gm.x_min = F(1); gm.y_max = F(2); gm.dx_rng = F(3); gm.dy_rng = F(4);
        gm.ksm1 = F(5); gm.ks = (int)q[6];
        const auto div_dy = udiv_by<HotMath>(gm.dy_rng, rcp_dy), div_dx = udiv_by<HotMath>(gm.dx_rng, rcp_dx);
        ACC* trr = tl_ + gm.ks * gm.ks;          // the R tile, from the block's ks
        SplatTaps tp;
        float sl, sr;
        if constexpr (TAB) {
            static_assert(!BIG && HotMath::kFused, "the weight table stands in for dp_weights_small<Lean> only");
            // the two table entries around x_tan: the load is in flight while the taps are computed (every lane loads,
            // also one whose ray misses the window: the index is clamped into the table whatever x_tan is)
            DpTableRef t;
            t.scale = F(7); t.tab = reinterpret_cast<const float2*>((uint64_t)q[8] | ((uint64_t)q[9] << 32));
            t.lo = F(10); t.hi = F(11); t.half = (int)q[12]; t.h = F(13); t.w = F(14);
            const float x_tan = HotMath::div(-dx, dz);
            float frac;
            const DpTablePair e = dp_table_fetch(t, x_tan, frac);
            if (!splat_taps<true>(gm, div_dy, div_dx, sx, sy, cx, cy, ra, tp)) return;
            dp_table_weights(t, e, frac, x_tan, sl, sr);
        } else {
            DevDpParams dp;
            dp.h = F(7); dp.f = F(8); dp.w = F(9); dp.r = F(10); dp.fmh = F(11); dp.rr = F(12);
            dp.inv_r = F(13); dp.r_pow2 = (int)q[14]; dp.tr = tr; dp.tl = tl; dp.big = BIG; dp.have_r = HAVE_R;
            if (!splat_taps<HotMath::kFused>(gm, div_dy, div_dx, sx, sy, cx, cy, ra, tp)) return;
            const float x_tan = HotMath::div(-dx, dz);
            if (BIG) dp_weights_big(dp, x_tan, sl, sr);      // separate instantiation: the rarely
            else dp_weights_small<HotMath>(dp, UDiv<HotMath>::make(dp.fmh), x_tan, sl, sr);   // used r > 0.5 branch costs registers
        }
        atomicAdd(&tl_[tp.i_tl], (ACC)(tp.w_tl * sl));
        atomicAdd(&tl_[tp.i_tr], (ACC)(tp.w_tr * sl));
        atomicAdd(&tl_[tp.i_bl], (ACC)(tp.w_bl * sl));
        atomicAdd(&tl_[tp.i_br], (ACC)(tp.w_br * sl));
        if (HAVE_R) {
            atomicAdd(&trr[tp.i_tl], (ACC)(tp.w_tl * sr));
            atomicAdd(&trr[tp.i_tr], (ACC)(tp.w_tr * sr));
            atomicAdd(&trr[tp.i_bl], (ACC)(tp.w_bl * sr));
            atomicAdd(&trr[tp.i_br], (ACC)(tp.w_br * sr));
        }
    };
    for_each_traced_ray<HotMath, THREADS, kPin, true>(
        lens, K, primary_trips, e, x2, y2, j * chunk + (int)threadIdx.x, s_end,
        by_work_left ? passes_p : kNoPrio, lds_mask, [&](const Ray& r) { splat(r.ox, r.oy, r.dx, r.dz, r.ra); });
    __builtin_amdgcn_s_setprio(0);               // (it is 0 already in a workgroup that never raised it)
    __syncthreads();

    // pstride: floats from one point's grid(s) to the next -- W * tile, or 2 * tile for SDIRT_PSF_INTERLEAVED
    // what the end of the workgroup needs of the loop block, read again: nothing of it was kept across the loops
    const u32x16 eq = sload_block(kernarg_at(kLoopAt));
    const int nsplit_e = (int)in_sgpr(eq[8]), K_e = (int)in_sgpr(eq[9]), ks_e = (int)in_sgpr(eq[12]), pstride = (int)in_sgpr(eq[13]);
    const int tile_e = ks_e * ks_e;
    ACC* trr = tiles + tile_e;
    float* Lg = lout + (int64_t)n * pstride + w * tile_e;
    float* Rg = HAVE_R ? rout + (int64_t)n * pstride + w * tile_e : nullptr;
    // (double tiles: every sum is rounded to fp32 ONCE here; the maximum and the quotients are taken of the rounded
    // values, i.e. of exactly what k_psf_normalize would read back)
    if (nsplit_e == 1) {
        if (flags & SDIRT_PSF_NORMALIZE) {
            float mx = -INFINITY;
            for (int i = threadIdx.x; i < tile_e; i += blockDim.x) mx = fmaxf(mx, (float)tl_[i]);
            const auto div_l = UDiv<HotMath>::make(block_max(mx, red) + 1e-6f);
            auto div_r = div_l;
            if (HAVE_R) {
                mx = -INFINITY;
                for (int i = threadIdx.x; i < tile_e; i += blockDim.x) mx = fmaxf(mx, (float)trr[i]);
                div_r = UDiv<HotMath>::make(block_max(mx, red) + 1e-6f);
            }
            for (int i = threadIdx.x; i < tile_e; i += blockDim.x) {
                Lg[i] = div_l((float)tl_[i]);
                if (HAVE_R) Rg[i] = div_r((float)trr[i]);
            }
        } else {
            for (int i = threadIdx.x; i < tile_e; i += blockDim.x) {
                Lg[i] = (float)tl_[i];
                if (HAVE_R) Rg[i] = (float)trr[i];
            }
        }
    } else {
        for (int i = threadIdx.x; i < tile_e; i += blockDim.x) {
            const float a = (float)tl_[i];
            if (a != 0.0f) atomicAdd(&Lg[i], a);
            if (HAVE_R) {
                const float b = (float)trr[i];
                if (b != 0.0f) atomicAdd(&Rg[i], b);
            }
        }
    }
    if (conv_mask && (int)threadIdx.x < K_e && lds_mask[threadIdx.x])
        atomicOr(&conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

static void launch_normalize(float* psf, int64_t N, int tile, hipStream_t st, int64_t stride = 0)
{
    const size_t lds = sizeof(float) * (size_t)tile;
    if (stride == 0) stride = tile;
    if (lds <= 48 * 1024 - 64)            // ks <= 110: inside the default dynamic-LDS allowance, two to ten workgroups per CU
        k_psf_normalize<true><<<(unsigned)N, kBlock, lds, st>>>(psf, tile, stride);
    else
        k_psf_normalize<false><<<(unsigned)N, kBlock, 0, st>>>(psf, tile, stride);
}

// first block of the last generation of a launch of `blocks` workgroups at four per CU (prio_by_work_left)
static int last_generation_from(int64_t blocks)
{
    return (int)std::max<int64_t>(0, blocks - 4ll * device_cus_or_default());
}

constexpr size_t kWideTilesMax = 39 * 1024;

static int spp_split(int64_t N, int64_t S, int* chunk_out, int n_cus = 0)
{
    // Fill the chip: at least ~4 workgroups per CU; split the spp axis when the
    // number of points alone cannot (e.g. PSFNet training: N=64, S=20000).
    int nsplit = 1;
    const int64_t want_blocks = (int64_t)(n_cus > 0 ? n_cus : device_cus_or_default()) * 4;
    if (N < want_blocks && S > 2 * kFused) {
        nsplit = (int)((want_blocks + N - 1) / N);
        const int max_split = (int)((S + 2 * kFused - 1) / (2 * kFused));
        if (nsplit > max_split) nsplit = max_split;
        if (nsplit < 1) nsplit = 1;
    }
    // slices of equal length up to a wave: a slice rounded up to whole workgroup passes (512) left the
    // last slice nearly empty and the CUs unevenly loaded (20000 spp: 13 x 1536 + 32 -> 16 x 1280, 17 % faster)
    int chunk = (int)((S + nsplit - 1) / nsplit);
    chunk = ((chunk + 63) / 64) * 64;
    nsplit = (int)((S + chunk - 1) / (chunk > 0 ? chunk : 1));
    if (nsplit < 1) nsplit = 1;
    if (chunk_out) *chunk_out = chunk;
    return nsplit;
}

// The chief-ray pass of the split path in slices: enough workgroups to touch every CU, at least
// one ray per lane and slice.
static int chief_slices(int64_t N, int64_t Sc, int* chunk_out)
{
    int64_t ns = std::min<int64_t>((Sc + kFused - 1) / kFused,
                                   (device_cus_or_default() + N - 1) / std::max<int64_t>(N, 1));
    if (ns < 1) ns = 1;
    int chunk = (int)((Sc + ns - 1) / ns);
    chunk = (chunk + 63) / 64 * 64;
    if (chunk < 64) chunk = 64;
    ns = (Sc + chunk - 1) / chunk;
    if (ns < 1) ns = 1;
    if (chunk_out) *chunk_out = chunk;
    return (int)ns;
}

// k_psf_lr's LDS tiles: float or double accumulators in workgroups of kFused, double ones in workgroups of
// 2 * kFused (SDIRT_PSF_DETERMINISTIC), float ones for the big-radius microlens branch
enum class Tiles { Float, Double, Double1024, BigFloat };

// One PSF call: the entry point's arguments, checked (check_psf_args), and how k_psf_lr runs them (plan_psf).
// W wavelength slots (W > 1 needs nsplit == 1): lens[w], trips[w], x2 / y2 [W][S], outputs [N][W][ks][ks], masks
// [W][SDIRT_MAX_SURFACES].  A chief-ray pass (`centered`) runs inside k_psf_lr when one workgroup owns a point
// (`fused`), as a launch of its own before it otherwise.
struct PsfLaunch {
    LensSet ls;
    TripSet tt, ttc;                 // primary and chief-ray trip tables
    int W, K, ks;
    int64_t N, S;
    const float* po;
    const float* x2;
    const float* y2;
    float pz, zs;
    uint32_t flags;
    const float* center;
    CenterArgs ca;                   // the chief-ray pass: xc / yc [W][Sc], center_out [W][N][2]
    bool centered;
    float* l;
    float* r;
    uint32_t* conv_mask;
    SplitArgs sa;
    hipStream_t st;
    const sdirt_lens* table_owner;   // the handle whose dual-pixel weight table the call may use: lens[0]
    bool strict_ieee;                // one of the call's handles is routed to the strict-IEEE kernels (routed_flags)
    // the plan
    SplatBlock sblk;
    DevDpParams dpp;
    bool both, interleaved, fused;
    bool tabbed;                     // the TAB instantiation: sblk carries the table's reference
    int nsplit, chunk, threads;
    Tiles tiles;
    size_t lds_bytes;
    int64_t pstride;
};

// What the PSF entry points share: pointers, sizes, the W primary lens tables (the surface count of lens_c if
// there is one, else of lens[0]), ks, dp and the trip tables.  primary = false: the chief-ray pass alone
// (sdirt_chief_center: no x2 / y2 / l_psf, no ks or dp).
static int check_psf_args(PsfLaunch& L, bool primary, const sdirt_lens* const* lens, int W, const sdirt_lens* lens_c,
                          const float* point_obj, int64_t N, const float* x2, const float* y2, int64_t S,
                          const float* xc, const float* yc, int64_t Sc, double pupil_z, double d_sensor, int ks,
                          const sdirt_dp_params* dp, const int32_t* trips, const int32_t* trips_c, const float* center,
                          const float* l_psf)
{
    if (!point_obj || !center || N < 0 || N > (1ll << 30) ||
        (primary && (!lens || W < 1 || W > SDIRT_MAX_WAVELENGTHS || !x2 || !y2 || !l_psf || S < 0 || S > (1ll << 30))) ||
        (lens_c && (!xc || !yc || Sc < 0 || Sc > (1ll << 30))) || (!primary && !lens_c))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    const sdirt_lens* ref = lens_c ? lens_c : lens[0];
    for (int w = 0; primary && w < W; ++w)
        if (!lens[w] || lens[w]->n_surfaces != ref->n_surfaces)
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "lens[%d] missing or surface count differs from %s", w,
                        lens_c ? "lens_center" : "lens[0]");
    if (primary) {
        if (int rc = check_ks(ks)) return rc;
        if (dp && !(dp->r > 0.0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->r must be > 0");
    }
    const int K = ref->n_surfaces;
    L = PsfLaunch{};
    if (primary) L.table_owner = lens[0];
    L.strict_ieee = (routed_flags(0u, lens_c) | (primary ? routed_flags(0u, lens, W) : 0u)) != 0u;
    for (int w = 0; primary && w < W; ++w) {
        L.ls.p[w] = lens[w]->dev;
        if (int rc = make_trips(lens[w], trips ? trips + (size_t)w * K : nullptr, L.tt.t[w])) return rc;
    }
    for (int w = 0; lens_c && w < std::max(W, 1); ++w)
        if (int rc = make_trips(lens_c, trips_c ? trips_c + (size_t)w * K : nullptr, L.ttc.t[w])) return rc;
    L.W = W; L.K = K; L.ks = ks; L.N = N; L.S = S;
    L.po = point_obj; L.x2 = x2; L.y2 = y2; L.pz = (float)pupil_z; L.zs = (float)d_sensor; L.center = center;
    if (lens_c) {
        L.centered = true;
        L.ca.lens_c = lens_c->dev; L.ca.xc = xc; L.ca.yc = yc; L.ca.Sc = (int)Sc;
    }
    return SDIRT_OK;
}

// The launch plan of a checked call: spp slices, the tile form, LDS and workgroup size -- or the refusal of
// SDIRT_PSF_INTERLEAVED / SDIRT_PSF_DETERMINISTIC.
static int plan_psf(PsfLaunch& L, double ps, const sdirt_dp_params* dp, uint32_t flags, float* l_psf, float* r_psf,
                    uint32_t* conv_mask, void* stream)
{
    const int tile = L.ks * L.ks;
    if (L.strict_ieee) flags |= SDIRT_PSF_STRICT_IEEE;
    L.flags = flags; L.l = l_psf; L.r = r_psf; L.conv_mask = conv_mask; L.st = as_stream(stream);
    // SDIRT_PSF_INTERLEAVED: l_psf / r_psf are the two halves of ONE [N, 2, ks, ks] array
    L.interleaved = (flags & SDIRT_PSF_INTERLEAVED) != 0;
    if (L.interleaved && (L.W != 1 || !dp || !r_psf || r_psf != l_psf + tile))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "SDIRT_PSF_INTERLEAVED: one wavelength, dp != NULL and r_psf == l_psf + ks * ks "
                                                "(the two halves of one [N, 2, ks, ks] array)");
    L.pstride = L.interleaved ? 2 * (int64_t)tile : (int64_t)L.W * tile;
    if ((int64_t)L.W * tile > (1ll << 30)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "grids too large");
    // a multi-wavelength launch keeps one workgroup per (point, wavelength): the chief-ray pass
    // stays fused and the whole of psf_rgb is one kernel, also for the few points of a psf_map
    L.chunk = ((int)L.S + kFused - 1) / kFused * kFused;
    L.nsplit = L.W > 1 ? 1 : spp_split(L.N, L.S, &L.chunk);
    L.fused = L.centered && L.nsplit == 1;
    L.dpp = make_dp(dp);
    // the weights from the sensor's table: the fused Lean small-radius case only (built or rebuilt on this stream, ahead
    // of the launch, when the handle's entries are another sensor's); else the closed form, as before
    DpTableRef tref;
    L.tabbed = !L.dpp.big && !(flags & SDIRT_PSF_STRICT_IEEE) && dp_table_enabled() && dp_table_for(L.table_owner, dp, L.st, tref);
    L.sblk = make_splat_block(make_geom(ps, L.ks), L.dpp, L.tabbed ? &tref : nullptr);
    L.both = r_psf != nullptr && L.dpp.have_r;
    // double accumulators (ACC of k_psf_lr) whenever they leave room for four workgroups per CU, i.e. for the
    // kernel's 8 waves per SIMD: 4 x (39 KiB + 0.4 KiB of static LDS) <= 160 KiB -- L + R up to ks 49, L alone up to 70
    const size_t n_acc = (size_t)tile * (L.both ? 2 : 1);
    // the corner-clipped microlens branch runs at 4 waves per SIMD whatever the tiles: float tiles only
    L.tiles = L.dpp.big ? Tiles::BigFloat : sizeof(double) * n_acc <= kWideTilesMax ? Tiles::Double : Tiles::Float;
    // SDIRT_PSF_DETERMINISTIC: double tiles also where only TWO workgroups per CU have room for them (L + R up to ks 70)
    // -- those then have 1024 threads; beyond that (or with the spp axis cut: partial grids meet in global float
    // atomics) there is no order-independent sum to offer
    if ((flags & SDIRT_PSF_DETERMINISTIC) && L.tiles != Tiles::Double) {
        if (L.dpp.big || L.nsplit > 1 || sizeof(double) * n_acc > 2 * kWideTilesMax)
            return fail(SDIRT_ERR_UNSUPPORTED, "SDIRT_PSF_DETERMINISTIC: float64 tiles need ks <= 70 (L + R; L alone: 99), r <= 0.5 and "
                                               "one workgroup per point (sdirt_psf_spp_slices == 1)");
        L.tiles = Tiles::Double1024;
    }
    if ((flags & SDIRT_PSF_DETERMINISTIC) && L.nsplit > 1)
        return fail(SDIRT_ERR_UNSUPPORTED, "SDIRT_PSF_DETERMINISTIC: the spp axis is cut for this batch (sdirt_psf_spp_slices > 1): "
                                           "partial grids are added with global float atomics");
    L.threads = L.tiles == Tiles::Double1024 ? 2 * kFused : kFused;
    L.lds_bytes = (L.tiles == Tiles::Float || L.tiles == Tiles::BigFloat ? sizeof(float) : sizeof(double)) * n_acc;
    if (L.fused) L.lds_bytes = std::max(L.lds_bytes, sizeof(double) * 3 * L.threads);  // fp64 reduction scratch
    return SDIRT_OK;
}

static LoopBlock make_loop_block(const PsfLaunch& L, int prio_from)
{
    LoopBlock b;
    std::memset(&b, 0, sizeof(b));
    b.x2 = L.x2; b.y2 = L.y2; b.po = L.po;
    b.S = (int32_t)L.S; b.chunk = L.chunk; b.nsplit = L.nsplit; b.K = L.K;
    b.pz = L.pz; b.zs = L.zs;
    b.ks = L.ks; b.pstride = (int32_t)L.pstride; b.prio_from = prio_from;
    return b;
}

static PrimarySet make_primary_set(const PsfLaunch& L)
{
    PrimarySet p;
    std::memset(&p, 0, sizeof(p));
    for (int w = 0; w < L.W; ++w) {
        p.s[w].t = L.tt.t[w];
        p.s[w].sb = L.sblk;
    }
    return p;
}

template <bool HAVE_R, bool BIG, class M, bool CENTER, class ACC, int THREADS, bool TAB = false>
static int launch_psf_lr_as(const PsfLaunch& L)
{
    constexpr auto kernel = &k_psf_lr<HAVE_R, BIG, M, CENTER, ACC, THREADS, TAB>;
    if (L.lds_bytes > 48 * 1024)        // large tiles: opt in to the full 160 KiB of LDS
        if (int rc = allow_large_lds<kernel>()) return rc;
    const dim3 grid((unsigned)(L.N * L.nsplit), (unsigned)L.W);
    kernel<<<grid, THREADS, L.lds_bytes, L.st>>>(
        L.sblk, make_loop_block(L, last_generation_from((int64_t)grid.x * grid.y)), make_primary_set(L), L.ttc, L.ls, L.dpp.tr, L.dpp.tl,
        L.center, L.flags, L.l, L.both ? L.r : nullptr, L.conv_mask, L.ca, L.sa);
    return SDIRT_OK;
}

// The one of k_psf_lr's 44 instantiations the plan asks for: tile form x HAVE_R x math x CENTER, and the twelve Lean
// small-radius ones once more with the weights from the table
static int launch_psf_lr(const PsfLaunch& L)
{
    return with_bool(L.both, [&](auto hr) { return with_bool(L.fused, [&](auto ct) { return with_math(L.flags, [&](auto m) {
        constexpr bool HR = decltype(hr)::value, CT = decltype(ct)::value;
        using M = decltype(m);
        if constexpr (M::kFused) {
            if (L.tabbed) switch (L.tiles) {
            case Tiles::Float: return launch_psf_lr_as<HR, false, M, CT, float, kFused, true>(L);
            case Tiles::Double: return launch_psf_lr_as<HR, false, M, CT, double, kFused, true>(L);
            case Tiles::Double1024: return launch_psf_lr_as<HR, false, M, CT, double, 2 * kFused, true>(L);
            case Tiles::BigFloat: return fail(SDIRT_ERR_UNSUPPORTED, "no weight table for r > 0.5");
            }
        }
        switch (L.tiles) {
        case Tiles::Float: return launch_psf_lr_as<HR, false, M, CT, float, kFused>(L);
        case Tiles::Double: return launch_psf_lr_as<HR, false, M, CT, double, kFused>(L);
        case Tiles::Double1024: return launch_psf_lr_as<HR, false, M, CT, double, 2 * kFused>(L);
        case Tiles::BigFloat: break;
        }
        return launch_psf_lr_as<HR, true, M, CT, float, kFused>(L);
    }); }); });
}

// `slope`: also the centre's derivative in the sensor plane (the SLOPE form of the kernel)
static int launch_chief_center(const PsfLaunch& L, double* slope = nullptr)
{
    with_math(L.flags, [&](auto m) { return with_bool(slope != nullptr, [&](auto sl) {
        k_chief_center<decltype(m), decltype(sl)::value><<<(int)L.N, kFused, 0, L.st>>>(
            L.ttc.t[0], L.ca.lens_c, L.K, L.po, L.ca.xc, L.ca.yc, L.ca.Sc, L.pz, L.zs, L.ca.center_out, slope,
            L.ca.any_valid, L.ca.conv_mask_c, last_generation_from(L.N));
        return 0;
    }); });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

// Uncentred, fused-centre and split-centre calls: [k_chief_center ->] k_psf_lr [-> normalisation].
static int launch_psf(PsfLaunch& L)
{
    const int tile = L.ks * L.ks;
    if (L.centered && !L.fused) {                // split spp axis: centre as its own launch
        if (int rc = launch_chief_center(L)) return rc;
        L.center = L.ca.center_out;
    }
    if (L.nsplit > 1) {
        HIP_TRY(hipMemsetAsync(L.l, 0, sizeof(float) * (size_t)L.N * tile * (L.interleaved ? 2 : 1), L.st));
        if (L.r && !L.interleaved) HIP_TRY(hipMemsetAsync(L.r, 0, sizeof(float) * (size_t)L.N * tile, L.st));
    }
    if (int rc = launch_psf_lr(L)) return rc;
    LAUNCH_CHECK();
    // param_list=None leaves the R grid all-zero (monte_carlo.py:230-235)
    if (!L.both && L.r) HIP_TRY(hipMemsetAsync(L.r, 0, sizeof(float) * (size_t)L.N * L.W * tile, L.st));
    if (L.nsplit > 1 && (L.flags & SDIRT_PSF_NORMALIZE)) {
        launch_normalize(L.l, L.N, tile, L.st, L.pstride);
        if (L.both) launch_normalize(L.r, L.N, tile, L.st, L.pstride);
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}

// A verified call on the split path, scratch = control block (zeroed by the caller) + chief-ray partial sums: round 1
// with the speculated tables, the tables checked on the device by the round's last kernel, round 2 with the corrected
// tables enqueued right behind it -- its kernels return at once when round 1 was right.  No host round trip in between.
// A round is k_chief_slices -> k_psf_lr -> k_psf_finish.
static int launch_psf_verified(PsfLaunch& L, uint32_t* ctl, double* part)
{
    if (L.nsplit == 1)
        return fail(SDIRT_ERR_UNSUPPORTED, "verified call: one workgroup per point here (sdirt_psf_spp_slices == 1); "
                                           "use sdirt_psf_lr_centered");
    const int tile = L.ks * L.ks;
    int chunk_c = 0;
    const int nslice_c = chief_slices(L.N, L.ca.Sc, &chunk_c);
    float* zr = (L.both && !L.interleaved) ? L.r : nullptr;      // interleaved: one run of N * 2 * tile floats
    const int64_t zn = L.N * tile * (L.interleaved ? 2 : 1);
    L.center = nullptr;
    L.sa.part = part;
    L.sa.nslice = nslice_c;
    const int rounds = (L.flags & SDIRT_PSF_ONE_ROUND) ? 1 : 2;
    for (int round = 0; round < rounds; ++round) {
        L.sa.gate = round ? ctl : nullptr;
        L.sa.trips_dev = round ? ctl + kCtlTrips2C : nullptr;
        uint32_t* mask_c = ctl + (round ? kCtlMask2C : kCtlMask1C);
        with_math(L.flags, [&](auto m) {
            k_chief_slices<decltype(m)><<<(int)(L.N * nslice_c), kFused, 0, L.st>>>(
                L.ttc.t[0], L.sa, L.ca.lens_c, L.K, L.po, L.ca.xc, L.ca.yc, L.ca.Sc, chunk_c, L.pz, L.zs, part,
                ctl + kCtlAnyValid, mask_c, L.l, zr, zn);
            return 0;
        });
        LAUNCH_CHECK();
        L.sa.trips_dev = round ? ctl + kCtlTrips2P : nullptr;
        L.conv_mask = ctl + (round ? kCtlMask2P : kCtlMask1P);
        if (int rc = launch_psf_lr(L)) return rc;
        LAUNCH_CHECK();
        FinishArgs fa;
        std::memset(&fa, 0, sizeof(fa));
        fa.gate = round ? ctl : nullptr;
        fa.ctl = round ? nullptr : ctl;
        fa.lens = L.ls.p[0]; fa.K = L.K; fa.tp = L.tt.t[0]; fa.tc = L.ttc.t[0];
        k_psf_finish<<<dim3((unsigned)L.N, L.both ? 2u : 1u), kBlock, 0, L.st>>>(
            L.l, L.r, tile, L.pstride, (L.flags & SDIRT_PSF_NORMALIZE) ? 1 : 0, fa);
        LAUNCH_CHECK();
    }
    // param_list=None leaves the R grid all-zero (monte_carlo.py:230-235)
    if (!L.both && L.r) HIP_TRY(hipMemsetAsync(L.r, 0, sizeof(float) * (size_t)L.N * tile, L.st));
    return SDIRT_OK;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

// How k_forward_integral_tiles is launched for N points x S samples on grids of ks x ks (ntile of them per point,
// `acc` bytes per accumulator).  false: the grids do not fit LDS.
static bool plan_forward_integral(int64_t N, int64_t S, int ks, int ntile, size_t acc, int ncu, FiLaunch& fl)
{
    const size_t lds_max = 160 * 1024 - 1024;
    fl.stride = (ntile * ks * ks) | 1;
    const size_t per_point = acc * (size_t)fl.stride;
    if (per_point > lds_max) return false;
    // one point per workgroup unless a point has fewer samples than the workgroup has threads (whole waves per
    // point: at most kFiThreads / 64 points), and never more than LDS holds
    int P = 1;
    while (P < kFiThreads / 64 && (int64_t)(kFiThreads / (2 * P)) >= S) P *= 2;
    while (P > 1 && (size_t)P * per_point > lds_max) P /= 2;
    fl.P = P;
    const int rp = kFiThreads / P;
    fl.logRp = 0;
    while ((1 << fl.logRp) < rp) ++fl.logRp;
    fl.ngroups = (int)((N + P - 1) / P);
    // few points: cut the spp axis as well, at least two passes per slice
    int64_t nsplit = 1;
    if (fl.ngroups < 2 * ncu) nsplit = std::min<int64_t>((2 * ncu + fl.ngroups - 1) / fl.ngroups, std::max<int64_t>(1, S / (2 * rp)));
    int64_t chunk = (S + nsplit - 1) / nsplit;
    chunk = std::max<int64_t>(rp, (chunk + rp - 1) / rp * rp);
    fl.chunk = chunk;
    fl.nsplit = (int)std::max<int64_t>(1, (S + chunk - 1) / chunk);
    return true;
}

int sdirt_forward_integral_plan(int64_t N, int64_t S, int32_t ks, int32_t both, int32_t n_cus, int64_t* plan)
{
    if (!plan || N < 1 || S < 1 || n_cus < 1) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = check_ks(ks, SDIRT_MAX_KS_STAGED)) return rc;
    FiLaunch fl;
    const int ntile = both ? 2 : 1;
    const bool wide = plan_forward_integral(N, S, ks, ntile, sizeof(double), n_cus, fl);
    const bool tiles = wide || plan_forward_integral(N, S, ks, ntile, sizeof(float), n_cus, fl);
    plan[0] = tiles ? (wide ? 8 : 4) : 0;
    for (int i = 1; i < 6; ++i) plan[i] = 0;
    if (!tiles) return SDIRT_OK;
    plan[1] = fl.P; plan[2] = fl.ngroups; plan[3] = fl.nsplit; plan[4] = fl.chunk;
    plan[5] = (int64_t)plan[0] * fl.P * fl.stride;
    return SDIRT_OK;
}

int sdirt_forward_integral(sdirt_rays rays, int64_t S, int64_t N, double ps, int32_t ks,
                           const float* center, const sdirt_dp_params* dp, uint32_t flags, float* l_grid,
                           float* r_grid, void* stream)
{
    if (int rc = check_rays(rays)) return rc;
    if (int rc = check_ks(ks, SDIRT_MAX_KS_STAGED)) return rc;
    if (!center || !l_grid || S < 0 || N < 0 || N > (1ll << 30)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (dp && !(dp->r > 0.0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->r must be > 0");
    if (N == 0) return SDIRT_OK;
    hipStream_t st = as_stream(stream);
    const size_t bytes = sizeof(float) * (size_t)N * ks * ks;
    const DevDpParams dpp = make_dp(dp);
    const bool both = r_grid != nullptr && dpp.have_r;
    FiLaunch fl;
    int ncu = 0;
    if (int rc = device_cus(&ncu)) return rc;
    const int ntile = both ? 2 : 1;
    // double accumulators when they fit (ks <= 99 for L + R), float ones up to SDIRT_MAX_KS, else the grids stay in HBM
    const bool wide = S > 0 && plan_forward_integral(N, S, ks, ntile, sizeof(double), ncu, fl);
    const bool tiles = wide || (S > 0 && plan_forward_integral(N, S, ks, ntile, sizeof(float), ncu, fl));
    // param_list=None leaves the R grid all-zero (monte_carlo.py:230-235); grids that are added to start at zero
    if (!tiles || fl.nsplit > 1) HIP_TRY(hipMemsetAsync(l_grid, 0, bytes, st));
    if (r_grid && (!tiles || fl.nsplit > 1 || !both)) HIP_TRY(hipMemsetAsync(r_grid, 0, bytes, st));
    if (S == 0) return SDIRT_OK;
    const bool normalize = (flags & SDIRT_PSF_NORMALIZE) != 0;
    if (!tiles) {
        k_forward_integral_hbm<<<grid_for(S * N, kBlock), kBlock, 0, st>>>(
            rays, S, N, make_geom(ps, ks), dpp, center, l_grid, r_grid);
        if (normalize) {
            launch_normalize(l_grid, N, ks * ks, st);
            if (both) launch_normalize(r_grid, N, ks * ks, st);
        }
        LAUNCH_CHECK();
        return SDIRT_OK;
    }
    const size_t lds_bytes = (wide ? sizeof(double) : sizeof(float)) * (size_t)fl.P * fl.stride;
    const unsigned grid = (unsigned)fl.ngroups * (unsigned)fl.nsplit;
    const int rc = with_bool(both, [&](auto hr) { return with_bool(dpp.big, [&](auto bg) {
        return with_bool(wide, [&](auto wd) { return with_math(flags, [&](auto m) -> int {
            constexpr auto kernel = &k_forward_integral_tiles<decltype(hr)::value, decltype(bg)::value,
                                                              std::conditional_t<decltype(wd)::value, double, float>, decltype(m)>;
            if (lds_bytes > 48 * 1024)
                if (int rc_ = allow_large_lds<kernel>()) return rc_;
            kernel<<<grid, kFiThreads, lds_bytes, st>>>(rays, S, N, make_geom(ps, ks), dpp, fl, center, l_grid,
                                                        both ? r_grid : nullptr, normalize ? 1 : 0);
            return SDIRT_OK;
        }); });
    }); });
    if (rc) return rc;
    if (normalize && fl.nsplit > 1) {          // the partial tiles have only just been added up in HBM
        launch_normalize(l_grid, N, ks * ks, st);
        if (both) launch_normalize(r_grid, N, ks * ks, st);
    }
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_dp_weight_table_selftest(const sdirt_lens* lens, const sdirt_dp_params* dp, const float* x_tan, int64_t n,
                                   float* lr_table, float* lr_closed, int32_t* info, void* stream)
{
    if (!lens || !x_tan || !lr_table || !lr_closed || n < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (dp && !(dp->r > 0.0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->r must be > 0");
    hipStream_t st = as_stream(stream);
    DpTableRef t;
    if (!dp_table_for(lens, dp, st, t))
        return fail(SDIRT_ERR_UNSUPPORTED, "no weight table for these parameters (r > 0.5, a degenerate or very steep sensor, or a capturing stream)");
    if (info) { info[0] = 2 * t.half + 1; info[1] = lens->dp_table.log2_scale; }
    if (n == 0) return SDIRT_OK;
    k_dp_weights_both<<<grid_for(n, kBlock), kBlock, 0, st>>>(t, make_dp(dp), x_tan, n, reinterpret_cast<float2*>(lr_table),
                                                              reinterpret_cast<float2*>(lr_closed));
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_psf_normalize(float* psf, int64_t N, int32_t ks, void* stream)
{
    if (!psf || N < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (ks < 1) return fail(SDIRT_ERR_INVALID_ARGUMENT, "ks < 1");
    if (N == 0) return SDIRT_OK;
    launch_normalize(psf, N, ks * ks, as_stream(stream));
    LAUNCH_CHECK();
    return SDIRT_OK;
}

// sdirt_chief_center and, with `slope`, sdirt_chief_center_slope
static int chief_center_entry(const sdirt_lens* lens, const float* point_obj, int64_t N, const float* xc, const float* yc,
                              int64_t Sc, double pupil_z, double d_sensor, const int32_t* trips, uint32_t flags,
                              float* center, double* slope, int32_t* any_valid, uint32_t* conv_mask, void* stream)
{
    PsfLaunch L;
    if (int rc = check_psf_args(L, false, nullptr, 0, lens, point_obj, N, nullptr, nullptr, 0, xc, yc, Sc, pupil_z,
                                d_sensor, 0, nullptr, nullptr, trips, center, nullptr))
        return rc;
    if (N == 0) return SDIRT_OK;
    L.flags = L.strict_ieee ? flags | SDIRT_PSF_STRICT_IEEE : flags; L.st = as_stream(stream);
    L.ca.center_out = center; L.ca.any_valid = any_valid; L.ca.conv_mask_c = conv_mask;
    return launch_chief_center(L, slope);
}

int sdirt_chief_center(const sdirt_lens* lens, const float* point_obj, int64_t N, const float* xc,
                       const float* yc, int64_t Sc, double pupil_z, double d_sensor,
                       const int32_t* trips, uint32_t flags, float* center, int32_t* any_valid,
                       uint32_t* conv_mask, void* stream)
{
    return chief_center_entry(lens, point_obj, N, xc, yc, Sc, pupil_z, d_sensor, trips, flags, center, nullptr, any_valid,
                              conv_mask, stream);
}

int sdirt_chief_center_slope(const sdirt_lens* lens, const float* point_obj, int64_t N, const float* xc,
                             const float* yc, int64_t Sc, double pupil_z, double d_sensor,
                             const int32_t* trips, uint32_t flags, float* center, double* slope, int32_t* any_valid,
                             uint32_t* conv_mask, void* stream)
{
    if (!slope) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null slope");
    return chief_center_entry(lens, point_obj, N, xc, yc, Sc, pupil_z, d_sensor, trips, flags, center, slope, any_valid,
                              conv_mask, stream);
}

int sdirt_psf_lr(const sdirt_lens* lens, const float* point_obj, int64_t N, const float* x2,
                 const float* y2, int64_t S, double pupil_z, double d_sensor, double ps, int32_t ks,
                 const float* center, const sdirt_dp_params* dp, const int32_t* trips,
                 uint32_t flags, float* l_psf, float* r_psf, uint32_t* conv_mask, void* stream)
{
    return sdirt_psf_rgb(&lens, 1, point_obj, N, x2, y2, S, pupil_z, d_sensor, ps, ks, center, dp, trips, flags,
                         l_psf, r_psf, conv_mask, stream);
}

int sdirt_psf_rgb(const sdirt_lens* const* lens, int32_t W, const float* point_obj, int64_t N, const float* x2,
                  const float* y2, int64_t S, double pupil_z, double d_sensor, double ps, int32_t ks,
                  const float* center, const sdirt_dp_params* dp, const int32_t* trips, uint32_t flags,
                  float* l_psf, float* r_psf, uint32_t* conv_mask, void* stream)
{
    PsfLaunch L;
    if (int rc = check_psf_args(L, true, lens, W, nullptr, point_obj, N, x2, y2, S, nullptr, nullptr, 0, pupil_z,
                                d_sensor, ks, dp, trips, nullptr, center, l_psf))
        return rc;
    if (N == 0) return SDIRT_OK;
    if (int rc = plan_psf(L, ps, dp, flags, l_psf, r_psf, conv_mask, stream)) return rc;
    return launch_psf(L);
}

int sdirt_psf_lr_centered(const sdirt_lens* lens, const sdirt_lens* lens_center,
                          const float* point_obj, int64_t N, const float* x2, const float* y2,
                          int64_t S, const float* xc, const float* yc, int64_t Sc, double pupil_z,
                          double d_sensor, double ps, int32_t ks, const sdirt_dp_params* dp,
                          const int32_t* trips, const int32_t* trips_center, uint32_t flags,
                          float* center, int32_t* any_valid, float* l_psf, float* r_psf,
                          uint32_t* conv_mask, uint32_t* conv_mask_center, void* stream)
{
    return sdirt_psf_rgb_centered(&lens, 1, lens_center, point_obj, N, x2, y2, S, xc, yc, Sc, pupil_z,
                                  d_sensor, ps, ks, dp, trips, trips_center, flags, center, any_valid,
                                  l_psf, r_psf, conv_mask, conv_mask_center, stream);
}

int sdirt_psf_rgb_centered(const sdirt_lens* const* lens, int32_t W, const sdirt_lens* lens_center,
                           const float* point_obj, int64_t N, const float* x2, const float* y2,
                           int64_t S, const float* xc, const float* yc, int64_t Sc, double pupil_z,
                           double d_sensor, double ps, int32_t ks, const sdirt_dp_params* dp,
                           const int32_t* trips, const int32_t* trips_center, uint32_t flags,
                           float* center, int32_t* any_valid, float* l_psf, float* r_psf,
                           uint32_t* conv_mask, uint32_t* conv_mask_center, void* stream)
{
    PsfLaunch L;
    if (!lens_center) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = check_psf_args(L, true, lens, W, lens_center, point_obj, N, x2, y2, S, xc, yc, Sc, pupil_z, d_sensor,
                                ks, dp, trips, trips_center, center, l_psf))
        return rc;
    if (N == 0) return SDIRT_OK;
    L.ca.center_out = center; L.ca.any_valid = any_valid; L.ca.conv_mask_c = conv_mask_center;
    if (int rc = plan_psf(L, ps, dp, flags, l_psf, r_psf, conv_mask, stream)) return rc;
    return launch_psf(L);
}

int32_t sdirt_psf_spp_slices(int64_t N, int64_t S, int32_t n_cus)
{
    if (N < 1 || S < 1) return 1;
    return spp_split(N, S, nullptr, n_cus);
}

static size_t ctl_bytes() { return (sizeof(uint32_t) * SDIRT_CTL_WORDS + 63) / 64 * 64; }

int64_t sdirt_psf_verified_scratch_bytes(int64_t N, int64_t Sc)
{
    if (N < 0 || Sc < 0) return -1;
    return (int64_t)ctl_bytes() + (int64_t)sizeof(double) * 3 * N * chief_slices(std::max<int64_t>(N, 1), Sc, nullptr);
}

int sdirt_psf_lr_verified(const sdirt_lens* lens, const sdirt_lens* lens_center, const float* point_obj,
                          int64_t N, const float* x2, const float* y2, int64_t S, const float* xc,
                          const float* yc, int64_t Sc, double pupil_z, double d_sensor, double ps, int32_t ks,
                          const sdirt_dp_params* dp, const int32_t* trips, const int32_t* trips_center,
                          uint32_t flags, float* center, float* l_psf, float* r_psf, void* scratch,
                          void* stream)
{
    if (!lens_center || !scratch) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (((uintptr_t)scratch) & 7) return fail(SDIRT_ERR_INVALID_ARGUMENT, "scratch must be 8-byte aligned");
    if (!trips || !trips_center) return fail(SDIRT_ERR_INVALID_ARGUMENT, "a verified call needs both speculated tables");
    PsfLaunch L;
    if (int rc = check_psf_args(L, true, &lens, 1, lens_center, point_obj, N, x2, y2, S, xc, yc, Sc, pupil_z, d_sensor,
                                ks, dp, trips, trips_center, center, l_psf))
        return rc;
    for (int k = 0; k < lens->n_surfaces; ++k)
        if (trips[k] < 0 || trips_center[k] < 0)
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "a verified call runs the reference's batch-wide counts: no negative (per-wave) entries");
    if (N == 0) return SDIRT_OK;
    L.ca.center_out = center;
    if (int rc = plan_psf(L, ps, dp, flags, l_psf, r_psf, nullptr, stream)) return rc;
    return launch_psf_verified(L, static_cast<uint32_t*>(scratch),
                               reinterpret_cast<double*>(static_cast<char*>(scratch) + ctl_bytes()));
}

static size_t align64(size_t n) { return (n + 63) / 64 * 64; }

int64_t sdirt_psf_call_scratch_bytes(int64_t N, int64_t S, int64_t Sc)
{
    if (N < 0 || S < 0 || Sc < 0) return -1;
    return (int64_t)align64((size_t)sdirt_psf_verified_scratch_bytes(N, Sc)) + (int64_t)sizeof(float) * 4 * (S + Sc);
}

int sdirt_psf_call(const sdirt_lens* lens, const sdirt_lens* lens_center, const float* point_obj, int64_t N,
                   const float* u_host, int64_t S, int64_t Sc, double pupil_r, double pupil_r_center,
                   double pupil_z, double d_sensor, double ps, int32_t ks, const sdirt_dp_params* dp,
                   const int32_t* trips, const int32_t* trips_center, uint32_t flags, float* center,
                   float* l_psf, float* r_psf, void* scratch, uint32_t* ctl_host, void* stream)
{
    if (!lens || !lens_center || !u_host || !scratch || N < 0 || S < 1 || Sc < 1 || S > (1ll << 30) || Sc > (1ll << 30))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (((uintptr_t)scratch) & 7) return fail(SDIRT_ERR_INVALID_ARGUMENT, "scratch must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    const int64_t n = 2 * (S + Sc);
    uint32_t* ctl = static_cast<uint32_t*>(scratch);
    float* u = reinterpret_cast<float*>(static_cast<char*>(scratch) +
                                        align64((size_t)sdirt_psf_verified_scratch_bytes(N, Sc)));
    float* xy = u + n;
    // The uniforms: page-locked host memory is mapped into the device's address space -- the mapping kernel reads them
    // where they are (48 KB over PCIe, a few microseconds) instead of behind a copy on the stream.  A copy command between
    // two kernels of one stream costs two engine hand-overs, compute queue -> SDMA engine -> compute queue: 12 us each, 25
    // of the 38 us a 2048-point step idled between its fused kernels (profiles/r06/step_timeline_plain.txt).  Memory that
    // is not mapped (pageable memory handed in against the contract) still goes through the copy.
    const float* u_src = nullptr;
    {
        void* mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, const_cast<float*>(u_host), 0) == hipSuccess && mapped)
            u_src = static_cast<const float*>(mapped);
        else
            (void)hipGetLastError();
    }
    if (!u_src) {
        HIP_TRY(hipMemcpyAsync(u, u_host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st));
        u_src = u;
    }
    // the reference's draw order (optics.py:483-484, then again inside psf_center): theta, r^2 of the primary
    // pass, theta, r^2 of the chief-ray pass -- both mappings (and SDIRT_PSF_ZERO_CTL) in one launch
    k_pupil_pair<<<grid_for(std::max<int64_t>(S + Sc, SDIRT_CTL_WORDS), kBlock, 1 << 30), kBlock, 0, st>>>(
        u_src, (int)S, (int)Sc, (float)(pupil_r * pupil_r), (float)(pupil_r_center * pupil_r_center), xy, ctl,
        (flags & SDIRT_PSF_ZERO_CTL) ? SDIRT_CTL_WORDS : 0);
    LAUNCH_CHECK();
    const uint32_t kflags = flags & ~(SDIRT_PSF_ZERO_CTL | SDIRT_PSF_NO_VERIFY);
    if (N == 0) {
        // an empty shard of a sharded batch: nothing to render, its (cleared) control block still enters the reductions
    } else if (spp_split(N, S, nullptr) > 1) {
        if (flags & SDIRT_PSF_NO_VERIFY)
            return fail(SDIRT_ERR_UNSUPPORTED, "SDIRT_PSF_NO_VERIFY: only for calls with one workgroup per point (sdirt_psf_spp_slices == 1)");
        if (int rc = sdirt_psf_lr_verified(lens, lens_center, point_obj, N, xy, xy + S, S, xy + 2 * S, xy + 2 * S + Sc, Sc,
                                           pupil_z, d_sensor, ps, ks, dp, trips, trips_center, kflags, center, l_psf, r_psf,
                                           scratch, stream))
            return rc;
    } else {
        // one workgroup per point: ONE fused launch with the speculated tables, its masks and the any-valid flag
        // straight into the control block, the trip rule evaluated behind it by one thread (status, corrected tables);
        // a correction is the caller's next call (SDIRT_PSF_ONE_ROUND is implied)
        if (!trips || !trips_center) return fail(SDIRT_ERR_INVALID_ARGUMENT, "sdirt_psf_call needs both speculated tables");
        if (int rc = sdirt_psf_lr_centered(lens, lens_center, point_obj, N, xy, xy + S, S, xy + 2 * S, xy + 2 * S + Sc, Sc,
                                           pupil_z, d_sensor, ps, ks, dp, trips, trips_center, kflags, center,
                                           reinterpret_cast<int32_t*>(ctl + kCtlAnyValid), l_psf, r_psf, ctl + kCtlMask1P,
                                           ctl + kCtlMask1C, stream))
            return rc;
        if (!(flags & SDIRT_PSF_NO_VERIFY)) {
            TripTable tp, tc;
            if (int rc = make_trips(lens, trips, tp)) return rc;
            if (int rc = make_trips(lens_center, trips_center, tc)) return rc;
            k_ctl_verify<<<1, 64, 0, st>>>(ctl, lens->dev, lens->n_surfaces, tp, tc);
            LAUNCH_CHECK();
        }
    }
    if (ctl_host)
        HIP_TRY(hipMemcpyAsync(ctl_host, scratch, sizeof(uint32_t) * SDIRT_CTL_WORDS, hipMemcpyDeviceToHost, st));
    return SDIRT_OK;
}

int sdirt_ctl_to_lanes(const uint32_t* ctl, uint32_t tag, int32_t* lanes, void* stream)
{
    if (!ctl || !lanes) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    k_ctl_to_lanes<<<grid_for(SDIRT_CTL_LANES, kBlock), kBlock, 0, as_stream(stream)>>>(ctl, tag, lanes);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_ctl_from_lanes(const int32_t* lanes, const sdirt_lens* lens, const int32_t* trips, const int32_t* trips_center,
                         uint32_t* ctl, uint32_t* ctl_host, void* stream)
{
    if (!lanes || !ctl || (lens && (!trips || !trips_center))) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    TripTable tp, tc;
    std::memset(&tp, 0, sizeof(tp));
    std::memset(&tc, 0, sizeof(tc));
    if (lens) {
        if (int rc = make_trips(lens, trips, tp)) return rc;
        if (int rc = make_trips(lens, trips_center, tc)) return rc;
    }
    hipStream_t st = as_stream(stream);
    k_ctl_from_lanes<<<1, 2 * SDIRT_MAX_SURFACES, 0, st>>>(lanes, ctl, lens ? lens->dev : nullptr, lens ? lens->n_surfaces : 0, tp, tc);
    LAUNCH_CHECK();
    if (ctl_host)
        HIP_TRY(hipMemcpyAsync(ctl_host, ctl, sizeof(uint32_t) * SDIRT_CTL_WORDS, hipMemcpyDeviceToHost, st));
    return SDIRT_OK;
}

}  // extern "C"
