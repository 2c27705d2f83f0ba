// sdirt_trace.hip -- lens tables and the STAGED ray API of libsdirt_dp.so (MI355X / gfx950 only):
// object points, pupil samples, SoA rays, sequential trace, propagation, centroid -- the kernels
// behind Lensgroup.sample_from_points / trace / trace2sensor / psf_center(rays) (deeplens/optics.py:
// 460-494, 601-717, 889-904).  The fused PSF kernels live in sdirt_psf.hip, the per-pixel
// convolutions in sdirt_render.hip.  See include/sdirt_dp.h for the ABI, DESIGN.md for layouts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/sdirt_dp.h"
#include "sdirt_trace.hpp"

using namespace sdirt;

// The largest fp32 X with sqrtf(X) <= r: a plane's aperture test sqrt(x^2 + y^2) <= r (surfaces.py:421) as
// x^2 + y^2 <= X, exactly, because the correctly rounded root is monotone.  X is NOT fl(r * r) in general (r = 5:
// one float above 25); it is found by stepping from there with the host's correctly rounded sqrtf.
static float plane_r2_max(float r)
{
    if (!(r >= 0.0f)) return r != r ? r : -1.0f;                 // NaN stays NaN; nothing passes a negative radius
    if (std::isinf(r)) return r;
    float x = r * r;
    if (std::isinf(x)) x = std::numeric_limits<float>::max();
    while (x > 0.0f && std::sqrt(x) > r) x = std::nextafter(x, 0.0f);
    for (float up = std::nextafter(x, INFINITY); !std::isinf(up) && std::sqrt(up) <= r; up = std::nextafter(x, INFINITY))
        x = up;
    return x;
}

// Can a curved surface with k > -1 and this curvature reach the one operand pair at which the seeded second quotient
// of the sag (sag_g_dgd, SEED2) misses the IEEE quotient: onesf = 1 + sf = kSeed2Onesf (its square rounds to the
// all-ones mantissa 0x3fffffff) under a power-of-two numerator fl(N c), N = fma(0.5, a / sf, onesf)?  Plain IEEE float
// arithmetic: sqrt_pos is the correctly rounded root (selftest mode 3), and N has the same bits under either seed of
// a / sf (mode 4).  onesf(a) does not increase with a, so the floats a of [0, 1) that map to kSeed2Onesf are found by
// bisection on the bit pattern and a walk -- there is one -- and each gives one N.  The aperture is not looked at: the
// answer holds for every ray.
constexpr uint32_t kSeed2Onesf = 0x3fb504f3u;
static float bits_float(uint32_t u) { float f; std::memcpy(&f, &u, sizeof f); return f; }
static uint32_t float_bits(float f) { uint32_t u; std::memcpy(&u, &f, sizeof u); return u; }
static bool sag_seed_exception(float c)
{
    const auto onesf_of = [](uint32_t abits) { return 1.0f + std::sqrt(1.0f - bits_float(abits)); };
    const float target = bits_float(kSeed2Onesf);
    uint32_t lo = 0u, hi = 0x3f800000u;                 // a = +0 (onesf = 2) ... a = 1 (onesf = 1)
    while (lo < hi) {                                   // the first a with onesf(a) <= target
        const uint32_t mid = lo + (hi - lo) / 2;
        if (onesf_of(mid) <= target) hi = mid; else lo = mid + 1;
    }
    for (uint32_t ab = lo; ab < 0x3f800000u && onesf_of(ab) == target; ++ab) {
        const float a = bits_float(ab), sf = std::sqrt(1.0f - a);
        const float n = std::fmaf(0.5f, a / sf, target) * c;
        if (n != 0.0f && std::isfinite(n) && (float_bits(n) & 0x007fffffu) == 0u) return true;
    }
    return false;
}

// Per-surface constant block; every double->float rounding happens here, at the
// same place the reference's torch scalar handling performs it.  needs_ieee: set where the surface is one of the
// few whose curvature can reach the seeded sag quotient's one exception (sag_seed_exception); never cleared.
static DevSurface make_dev_surface(const sdirt_surface_desc& in, bool& needs_ieee)
{
    DevSurface s;
    std::memset(&s, 0, sizeof(s));
    SurfHot& h = s.h;
    const int deg = in.kind == SDIRT_ASPHERE ? in.ai_degree : 0;
    h.d = in.d; h.c = in.c; h.k = in.k;
    h.r2_lim = (float)(in.r * in.r);
    h.c2 = in.c * in.c;
    h.onepk = 1.0f + in.k;
    if (in.kind != SDIRT_PLANE) {
        float rc = 1.0f / h.c2;                       // tensor.reciprocal()
        rc = rc * (float)(1.0 - 1e-9);                // * python float (1-EPSILON)
        h.lim_loose = rc / h.onepk;
        h.d_plus_R = in.d + 1.0f / in.c;
        h.d_plus_R_b = h.d_plus_R;
        h.lim_tight = in.k > -1.0f ? std::min(h.r2_lim, h.lim_loose) : h.r2_lim;
        if (in.k > -1.0f && sag_seed_exception(h.c)) needs_ieee = true;
    } else {
        h.lim_tight = (float)in.r;                    // planes: the aperture radius itself ...
        h.r2_lim = plane_r2_max(h.lim_tight);         // ... and the largest x^2 + y^2 whose root passes it
    }
    const double eta_f = in.n1 / in.n2, eta_b = in.n2 / in.n1;
    h.eta_f = (float)eta_f;  h.eta2_f = (float)(eta_f * eta_f);
    h.eta_b = (float)eta_b;  h.eta2_b = (float)(eta_b * eta_b);
    const bool do_refract = in.kind == SDIRT_PLANE ? (eta_f != 1.0) : true;
    h.flags = (uint32_t)in.kind | (do_refract ? kFlagRefract : 0u) | (in.k > -1.0f ? kFlagKgtM1 : 0u) |
              (in.c > 0.0f ? kFlagCpos : 0u) | (h.onepk == 1.0f ? kFlagUnitK : 0u) | ((uint32_t)deg << 8);
    h.flags |= visit_bits(h.flags);               // the path each half of a visit takes, decoded here once per surface
    for (int i = 0; i < kMaxAi; ++i) {
        s.p.ai[i] = i < deg ? in.ai[i] : 0.0f;
        s.p.kai[i] = (float)(i + 1) * s.p.ai[i];
    }
    return s;
}

// ---------------------------------------------------------------------------
// staged kernels
// ---------------------------------------------------------------------------
__global__ void k_points_to_object(const float* __restrict__ pts, int64_t N, float tf, float rl,
                                   float sw, float sh, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float depth = pts[3 * i + 2];
    const float scale = ((-depth) * tf) / rl;                 // optics.py:1305
    out[3 * i] = ((pts[3 * i] * scale) * sw) / 2.0f;          // optics.py:959
    out[3 * i + 1] = ((pts[3 * i + 1] * scale) * sh) / 2.0f;  // optics.py:960
    out[3 * i + 2] = depth;
}

__global__ void k_pupil_samples(const float* __restrict__ ut, const float* __restrict__ ur,
                                int64_t S, float pr2, float* __restrict__ x2,
                                float* __restrict__ y2)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    pupil_point(ut[s], ur[s], pr2, x2[s], y2[s]);
}

// sample_from_points (optics.py:486-494) into a point-major SoA bundle (ray (s, n) = element n S + s): a pure
// streaming WRITE (32 bytes per ray against 12 / S + 8 / N read), so the kernel is shaped for the store path.
// VEC: every thread makes FOUR consecutive samples of one point (S % 4 == 0, arrays 16-byte aligned) and stores
// each component as one dwordx4 -- a wave instruction writes 1 KiB contiguous; the (n, s) pair is divided out
// once per thread and then stepped.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_sample_rays(const float* __restrict__ po, int64_t N, const float* __restrict__ x2,
              const float* __restrict__ y2, int64_t S, float pz, sdirt_rays R)
{
    constexpr int W = VEC ? 4 : 1;
    const int64_t SQ = S / W, MQ = N * SQ;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= MQ) return;
    int64_t n = q / SQ, sq = q - n * SQ;
    const int64_t dn = stride / SQ, dsq = stride - dn * SQ;
    for (; q < MQ; q += stride) {
        const float px = po[3 * n], py = po[3 * n + 1], pzo = po[3 * n + 2];
        const int64_t i = n * S + sq * W;
        if (VEC) {
            const float4 xs = *reinterpret_cast<const float4*>(x2 + 4 * sq), ys = *reinterpret_cast<const float4*>(y2 + 4 * sq);
            const Ray r0 = make_ray(px, py, pzo, xs.x, ys.x, pz), r1 = make_ray(px, py, pzo, xs.y, ys.y, pz),
                      r2 = make_ray(px, py, pzo, xs.z, ys.z, pz), r3 = make_ray(px, py, pzo, xs.w, ys.w, pz);
            *reinterpret_cast<float4*>(R.ox + i) = make_float4(r0.ox, r1.ox, r2.ox, r3.ox);
            *reinterpret_cast<float4*>(R.oy + i) = make_float4(r0.oy, r1.oy, r2.oy, r3.oy);
            *reinterpret_cast<float4*>(R.oz + i) = make_float4(r0.oz, r1.oz, r2.oz, r3.oz);
            *reinterpret_cast<float4*>(R.dx + i) = make_float4(r0.dx, r1.dx, r2.dx, r3.dx);
            *reinterpret_cast<float4*>(R.dy + i) = make_float4(r0.dy, r1.dy, r2.dy, r3.dy);
            *reinterpret_cast<float4*>(R.dz + i) = make_float4(r0.dz, r1.dz, r2.dz, r3.dz);
            *reinterpret_cast<float4*>(R.ra + i) = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (R.obliq) *reinterpret_cast<float4*>(R.obliq + i) = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        } else {
            store_ray(R, i, make_ray(px, py, pzo, x2[sq], y2[sq], pz));
        }
        n += dn; sq += dsq;
        if (sq >= SQ) { sq -= SQ; n += 1; }
    }
}

// Element j of the reference's [S, N(, 3)] tensors <-> element of the bundle: the same index for a flat bundle
// (N <= 1), n S + s for a point-major one.
__device__ __forceinline__ int64_t soa_index(int64_t j, int64_t S, int64_t N)
{
    if (N <= 1) return j;
    const int64_t s = j / N, n = j - s * N;
    return n * S + s;
}

__global__ void k_rays_from_aos(const float* __restrict__ o, const float* __restrict__ d,
                                const float* __restrict__ ra, int64_t M, int64_t S, int64_t N, int normalize, sdirt_rays R)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M;
         j += (int64_t)gridDim.x * blockDim.x) {
        Ray r;
        r.ox = o[3 * j]; r.oy = o[3 * j + 1]; r.oz = o[3 * j + 2];
        r.dx = d[3 * j]; r.dy = d[3 * j + 1]; r.dz = d[3 * j + 2];
        if (normalize) normalize3<Ieee>(r.dx, r.dy, r.dz);
        r.ra = ra ? ra[j] : 1.0f;
        r.ob = 1.0f;
        store_ray(R, soa_index(j, S, N), r);
    }
}

__global__ void k_rays_to_aos(sdirt_rays R, int64_t M, int64_t S, int64_t N, float* __restrict__ o, float* __restrict__ d)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = soa_index(j, S, N);
        if (o) { o[3 * j] = R.ox[i]; o[3 * j + 1] = R.oy[i]; o[3 * j + 2] = R.oz[i]; }
        if (d) { d[3 * j] = R.dx[i]; d[3 * j + 1] = R.dy[i]; d[3 * j + 2] = R.dz[i]; }
    }
}

// R: the bundle read, W: the bundle written (the same arrays for an in-place trace: every ray is read before it is
// written, by the thread that writes it).
// TO_SENSOR: trace2sensor (optics.py:638-664) -- the traced ray is carried on to the plane z = z_sensor
// (Ray.propagate_to) before it is stored: one pass over the bundle instead of two.
template <bool FWD, class MP, bool PREFETCH, bool TO_SENSOR = false>
__global__ void __launch_bounds__(kBlock)
k_trace(TripTable trips /* kernarg offset 0 */, const DevSurface* __restrict__ lens, int K, int first,
        int last, sdirt_rays R, sdirt_rays W, int64_t M, uint32_t* __restrict__ conv_mask, float z_sensor)
{
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M;
         i += (int64_t)gridDim.x * blockDim.x) {
        Ray r = load_ray(R, i);
        trace_ray<FWD, MP, PREFETCH, false, false, /*WAVE*/ true>(lens, first, last, kernarg_at(0), r,
                                                                   conv_mask ? lds_mask : nullptr);
        if (TO_SENSOR) propagate_to<MP>(r, z_sensor);
        store_ray(W, i, r);
    }
    __syncthreads();
    if (conv_mask && (int)threadIdx.x < K && lds_mask[threadIdx.x])
        atomicOr(&conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

// Ray.propagate_to (basics.py:256-264) on SoA rays: reads 24, writes 12 bytes per ray and divides once -- a
// streaming kernel.  VEC: four rays per thread, every component moved as dwordx4 (M % 4 == 0, aligned arrays).
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_propagate(float z, sdirt_rays R, int64_t M)
{
    if (VEC) {
        const int64_t MQ = M / 4;
        for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < MQ; q += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = 4 * q;
            const float4 oz = *reinterpret_cast<const float4*>(R.oz + i), dz = *reinterpret_cast<const float4*>(R.dz + i);
            const float4 ox = *reinterpret_cast<const float4*>(R.ox + i), dx = *reinterpret_cast<const float4*>(R.dx + i);
            const float4 oy = *reinterpret_cast<const float4*>(R.oy + i), dy = *reinterpret_cast<const float4*>(R.dy + i);
            const float t0 = (z - oz.x) / dz.x, t1 = (z - oz.y) / dz.y, t2 = (z - oz.z) / dz.z, t3 = (z - oz.w) / dz.w;
            *reinterpret_cast<float4*>(R.ox + i) = make_float4(ox.x + dx.x * t0, ox.y + dx.y * t1, ox.z + dx.z * t2, ox.w + dx.w * t3);
            *reinterpret_cast<float4*>(R.oy + i) = make_float4(oy.x + dy.x * t0, oy.y + dy.y * t1, oy.z + dy.z * t2, oy.w + dy.w * t3);
            *reinterpret_cast<float4*>(R.oz + i) = make_float4(oz.x + dz.x * t0, oz.y + dz.y * t1, oz.z + dz.z * t2, oz.w + dz.w * t3);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M;
             i += (int64_t)gridDim.x * blockDim.x) {
            const float dz = R.dz[i];
            const float t = (z - R.oz[i]) / dz;
            R.ox[i] = R.ox[i] + R.dx[i] * t;
            R.oy[i] = R.oy[i] + R.dy[i] * t;
            R.oz[i] = R.oz[i] + dz * t;
        }
    }
}

// Centroid over the spp axis of a point-major bundle: one workgroup per point reads the point's contiguous run,
// fp64 partial sums per thread (samples s = t, t + 256, ...) reduced in a fixed tree order (deterministic).
__global__ void __launch_bounds__(kBlock)
k_center_from_rays(sdirt_rays R, int64_t S, int64_t N, float* __restrict__ center, int32_t* __restrict__ any_valid)
{
    __shared__ double red[3][kBlock];
    __shared__ int red_any;
    const int64_t n = blockIdx.x;
    if (threadIdx.x == 0) red_any = 0;
    __syncthreads();
    double sx = 0.0, sy = 0.0, sr = 0.0;
    int any = 0;
    for (int64_t s = threadIdx.x; s < S; s += kBlock) {
        const int64_t i = n * S + s;
        const float ra = R.ra[i];
        sx += (double)(R.ox[i] * ra);
        sy += (double)(R.oy[i] * ra);
        sr += (double)ra;
        any |= (ra == 1.0f);
    }
    red[0][threadIdx.x] = sx; red[1][threadIdx.x] = sy; red[2][threadIdx.x] = sr;
    if (any) red_any = 1;
    reduce_centroid<kBlock>(&red[0][0]);
    if (threadIdx.x == 0) {
        const float2 c = centre_from_sums(red[0][0], red[1][0], red[2][0]);
        center[2 * n] = c.x;
        center[2 * n + 1] = c.y;
        if (any_valid && red_any) atomicOr(any_valid, 1);
    }
}

// ---------------------------------------------------------------------------
// diagnostics: does the Lean math policy ever differ from IEEE?
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix32(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (uint32_t)x;
}

// mode 0: sqrt over EVERY fp32 bit pattern i in [first, first+count)  (exhaustive when
//         first = 0, count = 2^32);
// mode 1: division over pseudo-random operand pairs: mantissas uniform over all 2^23 values,
//         exponents uniform in [-exp_span, exp_span], random signs;
// mode 3: sqrt_pos over every fp32 bit pattern i in [first, first+count) inside [2^-100, 2^100];
// mode 2: division over mantissa pairs i in [first, first+count) of the 2^46 pairs
//         (a = 1.m_a, b = 1.m_b; exhaustive when first = 0, count = 2^46).
// out[0] = number of results whose bits differ from the IEEE result, out[1..] = up to 8
// offending operand bit patterns.
// mode 4: the sag's a / sqrt_pos(1 - a) under its two seeds -- v_rcp_f32 of the root (Lean::div) and the root's own
//         v_rsq_f32 (Lean::div_seeded) -- over every fp32 bit pattern i of a in [first, first+count) (exhaustive when
//         first = 0, count = 2^32), and what reads it, G(a) = fma(0.5, a / sf, 1 + sf) (sag_g_dgd).  Nothing here is
//         compared with IEEE: the question is whether the two seeds can be told apart.
//         out[0] = values checked; out[1] = a whose G differs in its bits where 1 - a is a positive normal float (the
//         INSIDE contract of sag_g_dgd); out[2] = a elsewhere whose G differs and is not NaN under both; out[3] = a
//         whose bare quotient differs (not NaN under both; informative); out[4], out[5], out[6] = the smallest bit
//         pattern counted in out[1], out[2], out[3] (all ones: none); out[7], out[8] = 0.
__global__ void k_selftest_math(int mode, uint64_t first, uint64_t count, int exp_span,
                                unsigned long long* __restrict__ out)
{
    unsigned long long bad = 0;
    unsigned long long n_checked = 0, n_inside = 0, n_outside = 0, n_quot = 0;       // mode 4
    for (uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < first + count;
         i += (uint64_t)gridDim.x * blockDim.x) {
        if (mode == 0) {
            const float x = __uint_as_float((uint32_t)i);
            const float a = Lean::sqrt(x), b = __builtin_sqrtf(x);
            const bool same = (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b);
            if (!same) {
                const unsigned long long k = atomicAdd(&out[0], 1ull);
                if (k < 8) out[1 + k] = i;
            }
        } else if (mode == 3) {
            // sqrt_pos (rsq + Markstein correction) over every fp32 bit pattern in the range it
            // is specified for, [2^-100, 2^100]
            const float x = __uint_as_float((uint32_t)i);
            if (x >= 0x1p-100f && x <= 0x1p100f &&
                __float_as_uint(Lean::sqrt_pos(x)) != __float_as_uint(__builtin_sqrtf(x))) {
                const unsigned long long k = atomicAdd(&out[0], 1ull);
                if (k < 8) out[1 + k] = i;
            }
        } else if (mode == 4) {
            const float a = __uint_as_float((uint32_t)i);
            const float x = 1.0f - a;
            float r;
            const float sf = Lean::sqrt_pos_rsq(x, r);
            const float onesf = 1.0f + sf;
            const float q_rcp = Lean::div(a, sf), q_rsq = Lean::div_seeded(a, sf, r);
            const float g_rcp = __builtin_fmaf(0.5f, q_rcp, onesf), g_rsq = __builtin_fmaf(0.5f, q_rsq, onesf);
            ++n_checked;
            if (__float_as_uint(g_rcp) != __float_as_uint(g_rsq)) {
                if (x >= 0x1p-126f && x < __builtin_inff()) {
                    ++n_inside;
                    atomicMin(&out[4], (unsigned long long)i);
                } else if (!(g_rcp != g_rcp && g_rsq != g_rsq)) {
                    ++n_outside;
                    atomicMin(&out[5], (unsigned long long)i);
                }
            }
            if (__float_as_uint(q_rcp) != __float_as_uint(q_rsq) && !(q_rcp != q_rcp && q_rsq != q_rsq)) {
                ++n_quot;
                atomicMin(&out[6], (unsigned long long)i);
            }
        } else if (mode == 2) {
            // exhaustive division: i enumerates ALL mantissa pairs, operands in [1, 2)
            const float a = __uint_as_float(0x3f800000u | (uint32_t)(i & 0x7fffffu));
            const float b = __uint_as_float(0x3f800000u | (uint32_t)((i >> 23) & 0x7fffffu));
            if (__float_as_uint(Lean::div(a, b)) != __float_as_uint(a / b)) {
                const unsigned long long k = atomicAdd(&out[0], 1ull);
                if (k < 8) out[1 + k] = ((unsigned long long)__float_as_uint(a) << 32) | __float_as_uint(b);
            }
        } else {
            const uint32_t h0 = mix32(2 * i + 1), h1 = mix32(2 * i + 2), h2 = mix32(~i);
            const int ea = 127 + (int)(h2 % (2 * exp_span + 1)) - exp_span;
            const int eb = 127 + (int)((h2 >> 8) % (2 * exp_span + 1)) - exp_span;
            const float a = __uint_as_float((h0 & 0x807fffffu) | ((uint32_t)ea << 23));
            const float b = __uint_as_float((h1 & 0x807fffffu) | ((uint32_t)eb << 23));
            const float q = Lean::div(a, b);
            if (__float_as_uint(q) != __float_as_uint(a / b)) {
                ++bad;
                const unsigned long long k = atomicAdd(&out[0], 1ull);
                if (k < 8) out[1 + k] = ((unsigned long long)__float_as_uint(a) << 32) | __float_as_uint(b);
            }
        }
    }
    (void)bad;
    if (mode == 4) {
        if (n_checked) atomicAdd(&out[0], n_checked);
        if (n_inside) atomicAdd(&out[1], n_inside);
        if (n_outside) atomicAdd(&out[2], n_outside);
        if (n_quot) atomicAdd(&out[3], n_quot);
    }
}

// mode 5: the sag's second quotient n / onesf^2 under its two seeds -- v_rcp_f32(onesf^2) (Lean::div) and the square of
//         the refined 1 / onesf (Lean::div_seeded; sag_g_dgd, SEED2) -- on the operands the k > -1 copies can hold: onesf
//         in [1, 2], every numerator mantissa (the recurrence scales exactly with the numerator's exponent and sign).
//         Stage A (k_selftest_seed2_a): onesf = 1 + j 2^-23 for j in [first, first + count) of [0, 2^23]; the set E of
//         those whose refined reciprocal of onesf^2 differs between the seeds.  exp_span = 1: EVERY onesf of the range
//         is put into E instead (the full scan of the pairs; a tool run, a range of at most kSeed2Cap at a time).
//         Stage B (k_selftest_seed2_b): every member of E under all 2^23 numerators 1.m, the two quotients bit for bit.
//         out[0] = onesf checked; out[1] = |E| (members beyond kSeed2Cap are counted and not run); out[2] = pairs
//         checked; out[3] = pairs that differ; out[4 .. 19] = up to 16 of them, onesf << 32 | numerator;
//         out[kSeed2Words ...] = the members of E (bit patterns of onesf), kSeed2Cap words, in no particular order.
constexpr int kSeed2Cap = 4096, kSeed2Words = 64, kSeed2Misses = 16;

__global__ void k_selftest_seed2_a(uint64_t first, uint64_t count, int all, unsigned long long* __restrict__ out)
{
    unsigned long long n_checked = 0;
    for (uint64_t j = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < first + count;
         j += (uint64_t)gridDim.x * blockDim.x) {
        const float onesf = __uint_as_float(0x3f800000u + (uint32_t)j);
        const float b = onesf * onesf;
        const float y1 = Lean::recip(onesf), s0 = y1 * y1;
        const float y_rcp = Lean::recip(b);
        const float y_sq = __builtin_fmaf(__builtin_fmaf(-b, s0, 1.0f), s0, s0);
        ++n_checked;
        if (all || __float_as_uint(y_rcp) != __float_as_uint(y_sq)) {
            const unsigned long long k = atomicAdd(&out[1], 1ull);
            if (k < (unsigned long long)kSeed2Cap) out[kSeed2Words + k] = __float_as_uint(onesf);
        }
    }
    if (n_checked) atomicAdd(&out[0], n_checked);
}

__global__ void k_selftest_seed2_b(unsigned long long* __restrict__ out)
{
    const unsigned long long ne = out[1] < (unsigned long long)kSeed2Cap ? out[1] : (unsigned long long)kSeed2Cap;
    const uint64_t total = (uint64_t)ne << 23;
    unsigned long long n_checked = 0, n_bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const float onesf = __uint_as_float((uint32_t)out[kSeed2Words + (i >> 23)]);
        const float n = __uint_as_float(0x3f800000u | (uint32_t)(i & 0x7fffffu));
        const float b = onesf * onesf;
        const float y1 = Lean::recip(onesf);
        const float q_rcp = Lean::div(n, b), q_sq = Lean::div_seeded(n, b, y1 * y1);
        ++n_checked;
        if (__float_as_uint(q_rcp) != __float_as_uint(q_sq)) {
            ++n_bad;
            const unsigned long long k = atomicAdd(&out[3], 1ull);
            if (k < (unsigned long long)kSeed2Misses)
                out[4 + k] = ((unsigned long long)__float_as_uint(onesf) << 32) | __float_as_uint(n);
        }
    }
    if (n_checked) atomicAdd(&out[2], n_checked);
    (void)n_bad;
}

// mode 6: the sag's a / sqrt_pos(1 - a), seeded with the root's v_rsq_f32, with and without the two fma that refine the
//         seed -- Lean::div_seeded and Lean::div_seeded_once -- over every fp32 bit pattern i of a in [first, first+count)
//         (exhaustive when first = 0, count = 2^32), and what reads it, G(a) = fma(0.5, a / sf, 1 + sf) (sag_g_dgd).
//         As in mode 4 nothing is compared with IEEE: can the two forms be told apart behind G?
//         out[0] = values checked; out[1], out[2] = a whose G differs in its bits where 1 - a is a positive normal float
//         (the INSIDE contract of sag_g_dgd), a >= 0 and a < 0; out[3] = a elsewhere whose G differs and is not NaN under
//         both; out[4] = a whose bare quotient differs (not NaN under both; informative); out[5], out[6], out[7] = the
//         smallest bit pattern counted in out[1], out[2], out[3] (all ones: none); out[8] = v_rsq_f32(1 - a) less the
//         correctly rounded 1 / sqrt(1 - a), in floats (a signed count), at a = kSeedOnceProbe, the one argument at which
//         a CPU restatement with a seed one float low told the forms apart; out[9] = the bits of that v_rsq_f32 (0: the
//         range leaves the probe out); out[kSeedOnceWords ...] = the a counted in out[4], the first kSeedOnceCap to
//         arrive, in no particular order.
constexpr int kSeedOnceCap = 4096, kSeedOnceWords = 64;
constexpr uint32_t kSeedOnceProbe = 0x3dc39c73u;

__global__ void k_selftest_seed_once(uint64_t first, uint64_t count, unsigned long long* __restrict__ out)
{
    unsigned long long n_checked = 0, n_pos = 0, n_neg = 0, n_outside = 0;
    for (uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < first + count;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const float a = __uint_as_float((uint32_t)i);
        const float x = 1.0f - a;
        float r;
        const float sf = Lean::sqrt_pos_rsq(x, r);
        const float onesf = 1.0f + sf;
        const float q_two = Lean::div_seeded(a, sf, r), q_once = Lean::div_seeded_once(a, sf, r);
        const float g_two = __builtin_fmaf(0.5f, q_two, onesf), g_once = __builtin_fmaf(0.5f, q_once, onesf);
        ++n_checked;
        if (__float_as_uint(g_two) != __float_as_uint(g_once)) {
            if (x >= 0x1p-126f && x < __builtin_inff()) {
                if (a >= 0.0f) {
                    ++n_pos;
                    atomicMin(&out[5], (unsigned long long)i);
                } else {
                    ++n_neg;
                    atomicMin(&out[6], (unsigned long long)i);
                }
            } else if (!(g_two != g_two && g_once != g_once)) {
                ++n_outside;
                atomicMin(&out[7], (unsigned long long)i);
            }
        }
        if (__float_as_uint(q_two) != __float_as_uint(q_once) && !(q_two != q_two && q_once != q_once)) {
            const unsigned long long k = atomicAdd(&out[4], 1ull);
            if (k < (unsigned long long)kSeedOnceCap) out[kSeedOnceWords + k] = i;
        }
        if ((uint32_t)i == kSeedOnceProbe) {
            const float exact = (float)(1.0 / __builtin_sqrt((double)x));      // one argument; the test restates it
            out[8] = (unsigned long long)((long long)__float_as_uint(r) - (long long)__float_as_uint(exact));
            out[9] = __float_as_uint(r);
        }
    }
    if (n_checked) atomicAdd(&out[0], n_checked);
    if (n_pos) atomicAdd(&out[1], n_pos);
    if (n_neg) atomicAdd(&out[2], n_neg);
    if (n_outside) atomicAdd(&out[3], n_outside);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int sdirt_abi_version(void) { return SDIRT_ABI_VERSION; }

const char* sdirt_last_error(void) { return g_err; }

int sdirt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sdirt_lens_create(const sdirt_surface_desc* surfaces, int32_t n_surfaces, sdirt_lens** out)
{
    if (!surfaces || !out) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (n_surfaces < 1 || n_surfaces > SDIRT_MAX_SURFACES)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_surfaces=%d outside [1,%d]", n_surfaces,
                    SDIRT_MAX_SURFACES);
    for (int i = 0; i < n_surfaces; ++i) {
        const sdirt_surface_desc& s = surfaces[i];
        if (s.kind < SDIRT_PLANE || s.kind > SDIRT_ASPHERE)
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "surface %d: unknown kind %d", i, s.kind);
        if (s.ai_degree < 0 || s.ai_degree > SDIRT_MAX_AI)
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "surface %d: ai_degree %d outside [0,%d]", i,
                        s.ai_degree, SDIRT_MAX_AI);
        if ((s.kind == SDIRT_PLANE) != (s.c == 0.0f))
            return fail(SDIRT_ERR_INVALID_ARGUMENT,
                        "surface %d: kind/curvature mismatch (plane <=> c == 0)", i);
        if (!(s.n1 > 0.0) || !(s.n2 > 0.0))
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "surface %d: refractive index <= 0", i);
    }
    sdirt_lens* L = new (std::nothrow) sdirt_lens();
    if (!L) return fail(SDIRT_ERR_HIP, "out of host memory");
    L->n_surfaces = n_surfaces;
    L->dev = nullptr;
    L->host.resize(n_surfaces);
    L->strict_ieee = false;
    for (int i = 0; i < n_surfaces; ++i) L->host[i] = make_dev_surface(surfaces[i], L->strict_ieee);
    hipError_t e = hipMalloc(&L->dev, sizeof(DevSurface) * n_surfaces);
    if (e == hipSuccess)
        e = hipMemcpy(L->dev, L->host.data(), sizeof(DevSurface) * n_surfaces,
                      hipMemcpyHostToDevice);
    // the dual-pixel weight table of the fused PSF kernel: room for it now, its entries on the first call that uses it
    if (e == hipSuccess) e = hipMalloc(&L->dp_table.dev, sizeof(float2) * (kDpTableEntries + 1));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L->dp_table.ready, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (L->dp_table.ready) (void)hipEventDestroy(L->dp_table.ready);
        if (L->dp_table.dev) (void)hipFree(L->dp_table.dev);
        if (L->dev) (void)hipFree(L->dev);
        delete L;
        return fail(e == hipErrorNoDevice ? SDIRT_ERR_NO_DEVICE : SDIRT_ERR_HIP,
                    "lens upload failed: %s", hipGetErrorString(e));
    }
    *out = L;
    return SDIRT_OK;
}

void sdirt_lens_destroy(sdirt_lens* lens)
{
    if (!lens) return;
    if (lens->dp_table.ready) (void)hipEventDestroy(lens->dp_table.ready);
    if (lens->dp_table.dev) (void)hipFree(lens->dp_table.dev);
    if (lens->dev) (void)hipFree(lens->dev);
    delete lens;
}

int32_t sdirt_lens_num_surfaces(const sdirt_lens* lens) { return lens ? lens->n_surfaces : 0; }

int32_t sdirt_lens_strict_ieee(const sdirt_lens* lens) { return lens && lens->strict_ieee ? 1 : 0; }

int sdirt_points_to_object(const float* points, int64_t N, double tan_hfov, double r_last,
                           double sensor_w, double sensor_h, float* point_obj, void* stream)
{
    if (!points || !point_obj || N < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (N == 0) return SDIRT_OK;
    k_points_to_object<<<grid_for(N, kBlock, 1 << 30), kBlock, 0, as_stream(stream)>>>(
        points, N, (float)tan_hfov, (float)r_last, (float)sensor_w, (float)sensor_h, point_obj);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_pupil_samples(const float* u_theta, const float* u_r2, int64_t S, double pupil_r,
                        float* x2, float* y2, void* stream)
{
    if (!u_theta || !u_r2 || !x2 || !y2 || S < 0)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (S == 0) return SDIRT_OK;
    k_pupil_samples<<<grid_for(S, kBlock, 1 << 30), kBlock, 0, as_stream(stream)>>>(
        u_theta, u_r2, S, (float)(pupil_r * pupil_r), x2, y2);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_sample_rays(const float* point_obj, int64_t N, const float* x2, const float* y2, int64_t S,
                      double pupil_z, sdirt_rays rays, void* stream)
{
    if (!point_obj || !x2 || !y2 || N < 0 || S < 0)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = check_rays(rays)) return rc;
    if (N * S == 0) return SDIRT_OK;
    // streaming kernels: ~8 workgroups per CU, the rest by grid stride (each thread keeps 128 bytes of stores in flight)
    if (S % 4 == 0 && rays_aligned16(rays) && (((uintptr_t)x2 | (uintptr_t)y2) & 15) == 0)
        k_sample_rays<true><<<grid_for(S / 4 * N, kBlock, 2048), kBlock, 0, as_stream(stream)>>>(
            point_obj, N, x2, y2, S, (float)pupil_z, rays);
    else
        k_sample_rays<false><<<grid_for(N * S, kBlock), kBlock, 0, as_stream(stream)>>>(
            point_obj, N, x2, y2, S, (float)pupil_z, rays);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_rays_from_aos(const float* o, const float* d, const float* ra, int64_t M, int64_t N, int32_t normalize,
                        sdirt_rays rays, void* stream)
{
    if (!o || !d || M < 0 || (N > 1 && M % N != 0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = check_rays(rays)) return rc;
    if (M == 0) return SDIRT_OK;
    k_rays_from_aos<<<grid_for(M, kBlock), kBlock, 0, as_stream(stream)>>>(o, d, ra, M, N > 1 ? M / N : M, N, normalize,
                                                                           rays);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_rays_to_aos(sdirt_rays rays, int64_t M, int64_t N, float* o, float* d, void* stream)
{
    if (M < 0 || (N > 1 && M % N != 0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (int rc = check_rays(rays)) return rc;
    if (M == 0 || (!o && !d)) return SDIRT_OK;
    k_rays_to_aos<<<grid_for(M, kBlock), kBlock, 0, as_stream(stream)>>>(rays, M, N > 1 ? M / N : M, N, o, d);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_trace(const sdirt_lens* lens, int32_t first, int32_t last, int32_t backward,
                const int32_t* trips, uint32_t flags, sdirt_rays rays, int64_t M,
                uint32_t* conv_mask, void* stream)
{
    return sdirt_trace_to(lens, first, last, backward, trips, flags, rays, rays, M, conv_mask, stream);
}

static int launch_trace(const sdirt_lens* lens, int32_t first, int32_t last, int32_t backward,
                        const int32_t* trips, uint32_t flags, sdirt_rays rays, sdirt_rays out, int64_t M,
                        uint32_t* conv_mask, void* stream, bool to_sensor, double z_sensor)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    flags = routed_flags(flags, lens);
    if (first < 0 || last > lens->n_surfaces || first > last)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "surface range [%d,%d) outside [0,%d]", first, last,
                    lens->n_surfaces);
    if (int rc = check_rays(rays)) return rc;
    if (int rc = check_rays(out)) return rc;
    if ((rays.obliq == nullptr) != (out.obliq == nullptr))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "obliq must be present in both bundles or in neither");
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    if (M < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_rays < 0");
    if (M == 0) return SDIRT_OK;
    if (first == last) {                       // nothing to trace: the output bundle is the input bundle
        if (out.ox != rays.ox) {
            hipStream_t st = as_stream(stream);
            const float* src[8] = {rays.ox, rays.oy, rays.oz, rays.dx, rays.dy, rays.dz, rays.ra, rays.obliq};
            float* dst[8] = {out.ox, out.oy, out.oz, out.dx, out.dy, out.dz, out.ra, out.obliq};
            for (int c = 0; c < 8; ++c)
                if (src[c] && dst[c] != src[c])
                    HIP_TRY(hipMemcpyAsync(dst[c], src[c], sizeof(float) * (size_t)M, hipMemcpyDeviceToDevice, st));
        }
        return to_sensor ? sdirt_propagate_to(z_sensor, out, M, stream) : SDIRT_OK;
    }
    const int grid = grid_for(M, kBlock);
    const bool prefetch = (flags & SDIRT_TRACE_NO_PREFETCH) == 0;
    const float zs = (float)z_sensor;
    // forward, prefetching loop only for trace2sensor (the self-test form has no use for it)
    if (to_sensor && (backward || !prefetch)) return fail(SDIRT_ERR_UNSUPPORTED, "trace2sensor traces forward with the prefetching loop");
    with_bool(!backward, [&](auto fw) { return with_bool(prefetch, [&](auto pf) { return with_bool(to_sensor, [&](auto ts) {
        return with_math(flags, [&](auto m) {
            // trace2sensor exists in the forward, prefetching form only (checked above): no other TS instantiation
            constexpr bool FW = decltype(fw)::value, PF = decltype(pf)::value, TS = decltype(ts)::value && FW && PF;
            k_trace<FW, decltype(m), PF, TS><<<grid, kBlock, 0, as_stream(stream)>>>(
                tt, lens->dev, lens->n_surfaces, first, last, rays, out, M, conv_mask, zs);
            return 0;
        });
    }); }); });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_trace_to(const sdirt_lens* lens, int32_t first, int32_t last, int32_t backward,
                   const int32_t* trips, uint32_t flags, sdirt_rays rays, sdirt_rays out, int64_t M,
                   uint32_t* conv_mask, void* stream)
{
    return launch_trace(lens, first, last, backward, trips, flags, rays, out, M, conv_mask, stream, false, 0.0);
}

int sdirt_trace2sensor(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, double d_sensor, sdirt_rays rays,
                       sdirt_rays out, int64_t M, uint32_t* conv_mask, void* stream)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    return launch_trace(lens, 0, lens->n_surfaces, 0, trips, flags, rays, out, M, conv_mask, stream, true, d_sensor);
}

int sdirt_propagate_to(double z, sdirt_rays rays, int64_t M, void* stream)
{
    if (int rc = check_rays(rays)) return rc;
    if (M <= 0) return M < 0 ? fail(SDIRT_ERR_INVALID_ARGUMENT, "n_rays < 0") : SDIRT_OK;
    if (M % 4 == 0 && rays_aligned16(rays))
        k_propagate<true><<<grid_for(M / 4, kBlock, 2048), kBlock, 0, as_stream(stream)>>>((float)z, rays, M);
    else
        k_propagate<false><<<grid_for(M, kBlock), kBlock, 0, as_stream(stream)>>>((float)z, rays, M);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_center_from_rays(sdirt_rays rays, int64_t S, int64_t N, float* center, int32_t* any_valid,
                           void* stream)
{
    if (int rc = check_rays(rays)) return rc;
    if (!center || S < 0 || N < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (N == 0) return SDIRT_OK;
    if (N > (1ll << 30)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_points too large");
    k_center_from_rays<<<(unsigned)N, kBlock, 0, as_stream(stream)>>>(rays, S, N, center, any_valid);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_selftest_math(int32_t mode, uint64_t first, uint64_t count, int32_t exp_span,
                        uint64_t* out, void* stream)
{
    if (!out || mode < 0 || mode > 6 || exp_span < 0 || exp_span > 60)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (mode == 6) {
        // bit patterns of ONE fp32, as mode 4; `out` holds kSeedOnceWords + kSeedOnceCap words
        if (first > (1ull << 32) || count > (1ull << 32) - first)
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "mode 6: [first, first+count) outside [0, 2^32)");
        HIP_TRY(hipMemsetAsync(out, 0, sizeof(uint64_t) * (kSeedOnceWords + kSeedOnceCap), as_stream(stream)));
        HIP_TRY(hipMemsetAsync(out + 5, 0xff, sizeof(uint64_t) * 3, as_stream(stream)));               // "none yet"
        if (count == 0) return SDIRT_OK;
        k_selftest_seed_once<<<256 * 32, 256, 0, as_stream(stream)>>>(first, count, (unsigned long long*)out);
        LAUNCH_CHECK();
        return SDIRT_OK;
    }
    if (mode == 5) {
        // onesf = 1 + j 2^-23, j in [first, first + count) of [0, 2^23]; `out` holds kSeed2Words + kSeed2Cap words
        if (exp_span > 1 || first > (1ull << 23) + 1 || count > (1ull << 23) + 1 - first || (exp_span == 1 && count > (uint64_t)kSeed2Cap))
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "mode 5: [first, first+count) outside [0, 2^23], or a full scan of more than %d "
                                                    "divisors in one call", kSeed2Cap);
        HIP_TRY(hipMemsetAsync(out, 0, sizeof(uint64_t) * (kSeed2Words + kSeed2Cap), as_stream(stream)));
        if (count == 0) return SDIRT_OK;
        k_selftest_seed2_a<<<256, 256, 0, as_stream(stream)>>>(first, count, exp_span, (unsigned long long*)out);
        k_selftest_seed2_b<<<256 * 32, 256, 0, as_stream(stream)>>>((unsigned long long*)out);
        LAUNCH_CHECK();
        return SDIRT_OK;
    }
    // mode 4 walks bit patterns of ONE fp32: nothing beyond 2^32 (the other modes keep the ranges they always took)
    if (mode == 4 && (first > (1ull << 32) || count > (1ull << 32) - first))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "mode 4: [first, first+count) outside [0, 2^32)");
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(uint64_t) * 9, as_stream(stream)));
    if (mode == 4) HIP_TRY(hipMemsetAsync(out + 4, 0xff, sizeof(uint64_t) * 3, as_stream(stream)));   // "none yet"
    if (count == 0) return SDIRT_OK;
    k_selftest_math<<<256 * 32, 256, 0, as_stream(stream)>>>(mode, first, count, exp_span,
                                                            (unsigned long long*)out);
    LAUNCH_CHECK();
    return SDIRT_OK;
}

}  // extern "C"
