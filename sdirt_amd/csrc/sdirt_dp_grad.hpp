// sdirt_dp_grad.hpp -- the derivative of the dual-pixel weights with respect to h, f, w, and the workgroup reduction
// its callers sum with: the device code sdirt_grad.hip (the splat's and the energy's backward) and
// sdirt_render_rt.hip (the layered render's backward into h, f, w) share.  One copy of the clamp rule:
// whatever fits the sensor model through the PSFs and through the ray-traced render differentiates the same function.
//
// Everything sits in an unnamed namespace, as it did in sdirt_grad.hip: DpGrad is a kernel argument there, and the
// kernels of that unit keep their symbols (and their ISA, function by function) only if its name is mangled as before.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/sdirt_dp.h"
#include "sdirt_host.hpp"

namespace {

using namespace sdirt;

constexpr int kGradThreads = 256;

// The float64 copies of the parameters the derivatives are evaluated at.
struct DpGrad {
    double h, f, w, r, fmh;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The workgroup's sum of every thread's acc[COMPS], stored at out[0 .. COMPS): the wave by shuffles, the waves 0 to 3
// through LDS.  Called by all threads of the workgroup.
template <int COMPS>
__device__ __forceinline__ void block_sum_store(const double (&acc)[COMPS], double* __restrict__ out)
{
    __shared__ double red[kGradThreads / 64][COMPS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < COMPS; ++c) {
        const double v = wave_sum(acc[c]);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < COMPS) {
        double v = 0.0;
        for (int k = 0; k < kGradThreads / 64; ++k) v += red[k][threadIdx.x];
        out[threadIdx.x] = v;
    }
}

__device__ __forceinline__ bool in_range(float x, float lo, float hi) { return x >= lo && x <= hi; }

// dA/dx of the segment area at x (inside [-r, r]): the chord -2 sqrt(r^2 - x^2)
__device__ __forceinline__ double chord(double r, double x)
{
    return -2.0 * sqrt(fmax((r - x) * (r + x), 0.0));
}

// d/d(h, f, w) of the boundary a*w - (f*t - a*w)*h/(f - h) projected through the microlens (monte_carlo.py:169-171),
// a = +1 (right), 0 (middle), -1 (left)
__device__ __forceinline__ void d_lens(const DpGrad& q, double t, double a, double d[3])
{
    const double D = q.fmh, u = q.f * t - a * q.w;
    d[0] = -u * q.f / (D * D);
    d[1] = -q.h * t / D + u * q.h / (D * D);
    d[2] = a * q.f / D;
}

// The clamp rule of Z_a, a = +1, 0, -1 (right, middle, left; k = 0, 1, 2), where s_r = Z_m - Z_r and s_l = Z_l - Z_m:
// any derivative of Z_a is c1 * dx1 + c2 * dx2, x1 = the lens-projected boundary and x2 = a*w - h*t the margin
// boundary (:186-188).  use(k, a, c1, c2) is called for k = 0, 1, 2.
//  small r (monte_carlo.py:169-206): Z = A(clamp(x1, -r, r)) - c2 - A(clamp(c2, -r, r)), c2 = clamp(x2, -0.5, 0.5)
//  big r (:278-338): Z = T(x1) - c2 - T(x2), T(x) = A(c) - r^2 seg(clamp(u, tr, tl)) - r cos(clamp(u, tr, tl)),
//       c = clamp(x, -0.5, 0.5), u = acos(c / r); with the u clamp open T's derivative is -dc (the area terms cancel),
//       closed it is A'(c) dc
// The clamp decisions are taken on the forward's fp32 values: x1f and x2f recomputed as dp_weights_big (which divides
// with '/') and dp_weights_small (div_fmh) compute them, and for big r the fp32 acos of the forward.  The chords are
// float64, at the float64 x1 and x2.  (A callable, not arrays c1[3], c2[3]: the user's terms stay in the iteration
// that computes x1, whose product (f t - a w) h d_lens shares.)
template <bool BIG, class M, class Div, class Use>
__device__ __forceinline__ void clamp_gates(const DevDpParams& p, const Div& div_fmh, const DpGrad& q, float x_tan,
                                            Use&& use)
{
    const float fx = p.f * x_tan, hx = p.h * x_tan;
    float x1f[3], x2f[3];
    if (BIG) {
        x1f[0] = p.w - ((fx - p.w) * p.h) / p.fmh;
        x1f[1] = ((-fx) * p.h) / p.fmh;
        x1f[2] = (-p.w) - ((fx + p.w) * p.h) / p.fmh;
    } else {
        x1f[0] = p.w - div_fmh((fx - p.w) * p.h);
        x1f[1] = div_fmh((-fx) * p.h);
        x1f[2] = (-p.w) - div_fmh((fx + p.w) * p.h);
    }
    x2f[0] = p.w - hx; x2f[1] = 0.0f - hx; x2f[2] = (-p.w) - hx;
    const double t = (double)x_tan;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = 1.0 - (double)k;                 // +1, 0, -1
        const double x1 = a * q.w - (q.f * t - a * q.w) * q.h / q.fmh;
        const double x2 = a * q.w - q.h * t;
        double c1, c2;
        if (BIG) {
            const bool g1 = in_range(x1f[k], -0.5f, 0.5f), g2 = in_range(x2f[k], -0.5f, 0.5f);
            const float u1 = __ocml_acos_f32(clampf(x1f[k], -0.5f, 0.5f) / p.r);
            const float u2 = __ocml_acos_f32(clampf(x2f[k], -0.5f, 0.5f) / p.r);
            const bool gu1 = in_range(u1, p.tr, p.tl), gu2 = in_range(u2, p.tr, p.tl);
            c1 = g1 ? (gu1 ? -1.0 : chord(q.r, x1)) : 0.0;
            c2 = g2 ? -1.0 - (gu2 ? -1.0 : chord(q.r, x2)) : 0.0;
        } else {
            const bool g1 = in_range(x1f[k], -p.r, p.r), g2 = in_range(x2f[k], -0.5f, 0.5f);
            const bool gi = in_range(clampf(x2f[k], -0.5f, 0.5f), -p.r, p.r);
            c1 = g1 ? chord(q.r, x1) : 0.0;
            c2 = g2 ? -1.0 - (gi ? chord(q.r, x2) : 0.0) : 0.0;
        }
        use(k, a, c1, c2);
    }
}

// d/d(h, f, w) of Z_a: dx1 = d_lens, dx2 = (-t, 0, a)
template <bool BIG, class M, class Div>
__device__ __forceinline__ void dz_boundaries(const DevDpParams& p, const Div& div_fmh, const DpGrad& q, float x_tan,
                                              double dZ[3][3])
{
    const double t = (double)x_tan;
    clamp_gates<BIG, M>(p, div_fmh, q, x_tan, [&](int k, double a, double c1, double c2) {
        double d1[3];
        d_lens(q, t, a, d1);
        const double d2[3] = {-t, 0.0, a};
#pragma unroll
        for (int j = 0; j < 3; ++j) dZ[k][j] = c1 * d1[j] + c2 * d2[j];
    });
}

DpGrad make_dp_grad(const sdirt_dp_params* dp)      // NULL: the reference's defaults, as make_dp
{
    const double h = dp ? dp->h : 0.78, f = dp ? dp->f : 1.44;
    return DpGrad{h, f, dp ? dp->w : 0.3, dp ? dp->r : 0.5, f - h};
}

}  // namespace
