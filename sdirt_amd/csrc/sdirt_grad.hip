// sdirt_grad.hip -- the backward pass of the splat stage (deeplens/monte_carlo.py:9-68, 135-240, 242-372): the
// gradients of a loss with respect to the dual-pixel parameters (h, f, w), the PSF centres, the sensor position and
// the sensor-plane rays, given its gradients with respect to the RAW left and right grids; and the energy of a point
// with its backward pass.  The microlens radius r carries no gradient (it is re-wrapped by torch.tensor(r) at :167, :274).
//
// Per ray (splat_ray): the window test, the four bilinear taps and the sub-pixel areas s_l, s_r are recomputed with the
// forward's own fp32 operations (the same rays in and out of the window, the same clamp decisions: clamp_gates), then
//   d/d(h, f, w) : ra * (gl . taps * ds_l/dtheta + gr . taps * ds_r/dtheta)
//   d/d(cx, cy)  : ra * (s_l * d(gl . taps)/dc + s_r * d(gr . taps)/dc)      (through the bilinear weights)
// in float64.  A segment area A(x) = r^2 (u - sin(2u)/2), u = acos(x/r), is differentiated by its chord,
// dA/dx = -2 sqrt(r^2 - x^2): no acos in the derivative, and 0 where |x| = r (the reference's autograd gives a
// non-finite value there).  Every torch.clamp passes the gradient where lo <= x <= hi and stops it outside.
//
// Launch: one workgroup per (point, slice of the spp axis) (block_slice).  The kernels that sum keep the ray terms in
// float64 registers and reduce them across the wave with shuffles, across the workgroup through LDS, to ONE float64
// partial per (point, slice) (block_sum_store).  No atomics: the gradients are the same bits from run to run.
//
// Each piece is written once and the five kernels are made of them:
//   k_forward_integral_grad<.., FOCUS>  splat_ray + dz_boundaries, summed: 5 components, 6 with the sensor position
//   k_forward_integral_grad_rays        splat_ray + dz_dt, stored per ray
//   k_dp_energy                         the sums of ra s_l, ra s_r and ra over ALL rays of a point
//   k_dp_energy_grad<.., PARTIAL, RAYS> its backward pass: dz_boundaries summed, or dz_dt stored per ray
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/sdirt_dp.h"
#include "sdirt_dp_grad.hpp"
#include "sdirt_host.hpp"

using namespace sdirt;

namespace {

constexpr int kGradComps = 5;                       // h, f, w, cx, cy
constexpr int kFocusComps = 6;                      // ... and the sensor position (k_forward_integral_grad<.., FOCUS>)
constexpr int kEnergyComps = 3;                     // sum ra s_l, sum ra s_r, sum ra; backward: h, f, w
constexpr int kGradLdsBytes = 48 * 1024;            // both grids staged in LDS up to ks 78

struct GradLaunch {
    int64_t chunk;        // samples per slice
    int nslices;          // slices of the spp axis per point
    double dwr_dcx;       // d(column fraction)/d(cx) = -ksm1 / dx_rng (times the ray's weight)
    double dwb_dcy;       // d(row fraction)/d(cy)    = -ksm1 / dy_rng
};

// One workgroup per (point n, slice j) of samples [s_begin, s_end): blockIdx.x = n * nslices + j, which is also the
// row of the workgroup's partial.
struct Slice {
    int64_t n, s_begin, s_end;
    int j;
};

__device__ __forceinline__ Slice block_slice(const GradLaunch& g, int64_t S)
{
    Slice b;
    b.n = blockIdx.x / (uint32_t)g.nslices;
    b.j = (int)(blockIdx.x - (uint32_t)b.n * g.nslices);
    b.s_begin = (int64_t)b.j * g.chunk;
    b.s_end = min(S, b.s_begin + g.chunk);
    return b;
}

// Window test and bilinear taps of one ray: splat_taps' operations, one by one (the same rays in the window, the
// same taps), keeping the row / column fractions and the weight the bilinear weights are made of.
struct GradTaps {
    int i_tl, i_tr, i_bl, i_br;
    float wb, wr, w;
};

template <class DivY, class DivX>
__device__ __forceinline__ bool grad_taps(const SplatGeom& gm, const DivY& div_dy, const DivX& div_dx, float sx,
                                          float sy, float cx, float cy, float ra, GradTaps& tp)
{
    float px = (-sx) - cx;
    float py = (-sy) - cy;
    float w = ra * (__builtin_fabsf(px) < gm.lim ? 1.0f : 0.0f);
    w = w * (__builtin_fabsf(py) < gm.lim ? 1.0f : 0.0f);
    if (!(w != 0.0f)) return false;
    px = px * w; py = py * w;
    const float pf0 = div_dy(py - gm.y_max) * gm.ksm1;
    const float pf1 = div_dx(px - gm.x_min) * gm.ksm1;
    const float fl0 = __builtin_floorf(pf0), fl1 = __builtin_floorf(pf1);
    tp.wb = pf0 - fl0; tp.wr = pf1 - fl1; tp.w = w;
    const int r0 = (int)fl0, c0 = (int)fl1;
    const int r1 = (int)__builtin_floorf(pf0 + 1.0f), c1 = (int)__builtin_floorf(pf1 + 1.0f);
    const int ks = gm.ks;
    tp.i_tl = r0 * ks + c0;
    tp.i_tr = r0 * ks + c1;
    tp.i_bl = r1 * ks + c0;
    tp.i_br = (r0 + 1) * ks + (c0 + 1);
    return r0 >= 0 && c0 >= 0 && r1 < ks && c1 < ks && (r0 + 1) < ks && (c0 + 1) < ks;
}

// d/dt of Z_a, t = x_tan: dx1/dt = -f h / (f - h) and dx2/dt = -h -- what a ray's direction gets through
// x_tan = -d.x / d.z.
template <bool BIG, class M, class Div>
__device__ __forceinline__ void dz_dt(const DevDpParams& p, const Div& div_fmh, const DpGrad& q, float x_tan, double dT[3])
{
    const double d1 = -q.f * q.h / q.fmh, d2 = -q.h;
    clamp_gates<BIG, M>(p, div_fmh, q, x_tan, [&](int k, double, double c1, double c2) { dT[k] = c1 * d1 + c2 * d2; });
}

// The point's two upstream grids into LDS, [tile] left then [tile] right, a null grid as zeros.
__device__ __forceinline__ void stage_grids(const float* GL, const float* GR, int tile, float* lds)
{
    for (int e = threadIdx.x; e < tile; e += kGradThreads) {
        lds[e] = GL ? GL[e] : 0.0f;
        lds[tile + e] = GR ? GR[e] : 0.0f;
    }
    __syncthreads();
}

// What one ray in the window, with weight, hands to the kernel's tail.
struct RayTerms {
    float x_tan;          // (-d.x) / d.z (monte_carlo.py:48)
    double w;             // the ray's weight
    double bl, br;        // g . bilinear weights, left and right grid
    double g_x, g_y;      // the ray's terms of dLoss/d(cx, cy): the centre moves the shifted point (times the weight,
};                        // :38) and so the bilinear fractions

// The adjoint of the splat for one ray: the window test and taps, the forward's fp32 sub-pixel weights, the upstream
// gradients at the four taps (STAGE: from LDS; else through L2, a null grid read as 0) and the bilinear terms; then
// tail(RayTerms), in the same region.  A ray without weight or outside the window: no call.
template <bool BIG, class M, bool STAGE, class Tail>
__device__ __forceinline__ void splat_ray(const SplatGeom& gm, const DevDpParams& dp, const GradLaunch& gl_,
                                          const UDiv<M>& div_dy, const UDiv<M>& div_dx, const UDiv<M>& div_fmh,
                                          const float* GL, const float* GR, const float* g_lds, float cx, float cy,
                                          float ox, float oy, float dx, float dz, float ra, Tail&& tail)
{
    // d.x and d.z are first used behind the window test.  Left alone, the compiler sinks their loads there in some
    // instantiations (small r, lean, staged), and every ray in the window pays a second round trip to memory; this
    // keeps a ray's loads together in front of the test.
    asm volatile("" :: "v"(dx), "v"(dz));
    GradTaps tp;
    if (!grad_taps(gm, div_dy, div_dx, ox, oy, cx, cy, ra, tp)) return;
    const float x_tan = (-dx) / dz;
    float sl, sr;
    if (BIG) dp_weights_big(dp, x_tan, sl, sr);
    else dp_weights_small<M>(dp, div_fmh, x_tan, sl, sr);
    double lt, lr_, lb, lbr, rt = 0.0, rr_ = 0.0, rb = 0.0, rbr = 0.0;
    if (STAGE) {
        const int tile = gm.ks * gm.ks;
        lt = g_lds[tp.i_tl]; lr_ = g_lds[tp.i_tr]; lb = g_lds[tp.i_bl]; lbr = g_lds[tp.i_br];
        rt = g_lds[tile + tp.i_tl]; rr_ = g_lds[tile + tp.i_tr]; rb = g_lds[tile + tp.i_bl];
        rbr = g_lds[tile + tp.i_br];
    } else {
        lt = GL ? GL[tp.i_tl] : 0.0f; lr_ = GL ? GL[tp.i_tr] : 0.0f;
        lb = GL ? GL[tp.i_bl] : 0.0f; lbr = GL ? GL[tp.i_br] : 0.0f;
        if (GR) { rt = GR[tp.i_tl]; rr_ = GR[tp.i_tr]; rb = GR[tp.i_bl]; rbr = GR[tp.i_br]; }
    }
    const double wb = tp.wb, wr = tp.wr, w = tp.w;
    // g . bilinear weights, and its derivatives by the column (wr) and row (wb) fractions
    const double bl = (1.0 - wb) * ((1.0 - wr) * lt + wr * lr_) + wb * ((1.0 - wr) * lb + wr * lbr);
    const double br = (1.0 - wb) * ((1.0 - wr) * rt + wr * rr_) + wb * ((1.0 - wr) * rb + wr * rbr);
    const double bl_wr = (1.0 - wb) * (lr_ - lt) + wb * (lbr - lb), bl_wb = (1.0 - wr) * (lb - lt) + wr * (lbr - lr_);
    const double br_wr = (1.0 - wb) * (rr_ - rt) + wb * (rbr - rb), br_wb = (1.0 - wr) * (rb - rt) + wr * (rbr - rr_);
    const double cs = w * ((double)sl * bl_wr + (double)sr * br_wr), cr = w * ((double)sl * bl_wb + (double)sr * br_wb);
    tail(RayTerms{x_tan, w, bl, br, w * gl_.dwr_dcx * cs, w * gl_.dwb_dcy * cr});
}

// The ray terms summed: partial [N, nslices, 5] = d/d(h, f, w, cx, cy).  LDS: the point's two upstream grids (STAGE:
// they fit; else they are read through L2) and the per-wave sums.
// FOCUS: a SIXTH component, the sensor position s (the focus setting): the sensor-plane point of a ray is
// o = o' + d (s - o'.z) / d.z, so d(o.xy)/ds = d.xy / d.z, and o enters the splat as the centre does (the shift is
// -o - c): component 5 = sum over the rays of g_x d.x / d.z + g_y d.y / d.z.  The slopes and the sum are float64, from
// the forward's fp32 d; x_tan = -d.x / d.z and ra do not depend on s.  24 bytes per ray (d.y as well) instead of 20.
// Components 0 to 4 are the same operations in the same order with and without FOCUS: the same bits.
template <bool BIG, class M, bool STAGE, bool FOCUS>
__global__ void __launch_bounds__(kGradThreads)
k_forward_integral_grad(sdirt_rays R, int64_t S, SplatGeom gm, DevDpParams dp, DpGrad q, GradLaunch gl_,
                        const float* __restrict__ center, const float* __restrict__ gl, const float* __restrict__ gr,
                        double* __restrict__ partial)
{
    constexpr int COMPS = FOCUS ? kFocusComps : kGradComps;
    extern __shared__ __attribute__((aligned(16))) float g_lds[];
    const Slice b = block_slice(gl_, S);
    const int tile = gm.ks * gm.ks;
    const float* GL = gl ? gl + b.n * tile : nullptr;
    const float* GR = gr ? gr + b.n * tile : nullptr;
    if (STAGE) stage_grids(GL, GR, tile, g_lds);
    const float cx = center[2 * b.n], cy = center[2 * b.n + 1];
    const auto div_dy = UDiv<M>::make(gm.dy_rng), div_dx = UDiv<M>::make(gm.dx_rng);
    const auto div_fmh = UDiv<M>::make(dp.fmh);
    double acc[COMPS] = {};
    for (int64_t s = b.s_begin + threadIdx.x; s < b.s_end; s += kGradThreads) {
        const int64_t i = b.n * S + s;
        const float ox = R.ox[i], oy = R.oy[i], dx = R.dx[i], dz = R.dz[i], ra = R.ra[i];
        float dy = 0.0f;
        if constexpr (FOCUS) dy = R.dy[i];
        splat_ray<BIG, M, STAGE>(gm, dp, gl_, div_dy, div_dx, div_fmh, GL, GR, g_lds, cx, cy, ox, oy, dx, dz, ra,
                                 [&](const RayTerms& t) {
            double dZ[3][3];
            dz_boundaries<BIG, M>(dp, div_fmh, q, t.x_tan, dZ);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double dsr = dZ[1][c] - dZ[0][c], dsl = dZ[2][c] - dZ[1][c];
                acc[c] += t.w * (t.bl * dsl + t.br * dsr);
            }
            acc[3] += t.g_x;
            acc[4] += t.g_y;
            if constexpr (FOCUS) {      // the sensor plane moves the ray's point along the ray
                const double z = (double)dz;
                acc[5] += t.g_x * ((double)dx / z) + t.g_y * ((double)dy / z);
            }
        });
    }
    block_sum_store<COMPS>(acc, partial + (b.n * gl_.nslices + b.j) * COMPS);
}

// The per-ray terms k_forward_integral_grad sums, stored instead: ray_grad [4, M] = dLoss/d(o.x, o.y, d.x, d.z) of the
// sensor-plane rays (0 for a ray without weight or outside the window).  o.x / o.y enter as the centre does
// (points = -o.xy - centre, times the weight): the centre terms of that kernel, ray by ray; d.x / d.z through
// x_tan = -d.x / d.z.  The same launch geometry and LDS staging as k_forward_integral_grad; no reduction.
template <bool BIG, class M, bool STAGE>
__global__ void __launch_bounds__(kGradThreads)
k_forward_integral_grad_rays(sdirt_rays R, int64_t S, int64_t Mtot, SplatGeom gm, DevDpParams dp, DpGrad q, GradLaunch gl_,
                             const float* __restrict__ center, const float* __restrict__ gl, const float* __restrict__ gr,
                             float* __restrict__ ray_grad)
{
    extern __shared__ __attribute__((aligned(16))) float g_lds[];
    const Slice b = block_slice(gl_, S);
    const int tile = gm.ks * gm.ks;
    const float* GL = gl ? gl + b.n * tile : nullptr;
    const float* GR = gr ? gr + b.n * tile : nullptr;
    if (STAGE) stage_grids(GL, GR, tile, g_lds);
    const float cx = center[2 * b.n], cy = center[2 * b.n + 1];
    const auto div_dy = UDiv<M>::make(gm.dy_rng), div_dx = UDiv<M>::make(gm.dx_rng);
    const auto div_fmh = UDiv<M>::make(dp.fmh);
    for (int64_t s = b.s_begin + threadIdx.x; s < b.s_end; s += kGradThreads) {
        const int64_t i = b.n * S + s;
        const float ox = R.ox[i], oy = R.oy[i], dx = R.dx[i], dz = R.dz[i], ra = R.ra[i];
        float g_ox = 0.0f, g_oy = 0.0f, g_dx = 0.0f, g_dz = 0.0f;
        splat_ray<BIG, M, STAGE>(gm, dp, gl_, div_dy, div_dx, div_fmh, GL, GR, g_lds, cx, cy, ox, oy, dx, dz, ra,
                                 [&](const RayTerms& t) {
            double dT[3];
            dz_dt<BIG, M>(dp, div_fmh, q, t.x_tan, dT);
            const double dt = t.w * (t.bl * (dT[2] - dT[1]) + t.br * (dT[1] - dT[0]));          // dLoss/d(x_tan)
            const double z = (double)dz;
            g_ox = (float)t.g_x;
            g_oy = (float)t.g_y;
            g_dx = (float)(-dt / z);
            g_dz = (float)(dt * (double)dx / (z * z));
        });
        ray_grad[i] = g_ox; ray_grad[Mtot + i] = g_oy; ray_grad[2 * Mtot + i] = g_dx; ray_grad[3 * Mtot + i] = g_dz;
    }
}

// The energy of a point: E[n] = (sum ra s_l(x_tan), sum ra s_r(x_tan), sum ra) over ALL its spp rays, in the window or
// not -- what the raw grids would sum to if forward_integral did not zero the rays outside its window
// (monte_carlo.py:37-38; the four bilinear taps of a ray sum to 1), and what psf_diff computes as lum and drops
// (optics.py:979-991).  s_l, s_r are the splat's own fp32 weights (dp_weights_small<M> / dp_weights_big on
// x_tan = (-d.x) / d.z); the products and sums are float64, a thread's rays in order: one partial of 3 values per
// (point, slice).  12 bytes per ray.
template <bool BIG, class M>
__global__ void __launch_bounds__(kGradThreads)
k_dp_energy(sdirt_rays R, int64_t S, DevDpParams dp, GradLaunch gl_, double* __restrict__ partial)
{
    const Slice b = block_slice(gl_, S);
    const auto div_fmh = UDiv<M>::make(dp.fmh);
    double acc[kEnergyComps] = {};
    for (int64_t s = b.s_begin + threadIdx.x; s < b.s_end; s += kGradThreads) {
        const int64_t i = b.n * S + s;
        const float dx = R.dx[i], dz = R.dz[i], ra = R.ra[i];
        if (!(ra != 0.0f)) continue;
        const float x_tan = (-dx) / dz;                   // monte_carlo.py:48
        float sl, sr;
        if (BIG) dp_weights_big(dp, x_tan, sl, sr);
        else dp_weights_small<M>(dp, div_fmh, x_tan, sl, sr);
        const double w = ra;
        acc[0] += w * (double)sl;
        acc[1] += w * (double)sr;
        acc[2] += w;
    }
    block_sum_store<kEnergyComps>(acc, partial + (b.n * gl_.nslices + b.j) * kEnergyComps);
}

// The backward pass of k_dp_energy: given grad_e [N, 3] = dLoss/dE (column 2 is not read: ra is a forward decision),
//   partial  [N, nslices, 3] = sum over the slice's rays of ra (g_l ds_l/dtheta + g_r ds_r/dtheta), theta = h, f, w
//            (dz_boundaries: the derivatives and clamp rule of k_forward_integral_grad), and / or
//   ray_grad [4, M]: rows 2 and 3 = dLoss/d(d.x, d.z) through x_tan = -d.x / d.z (dz_dt, as
//            k_forward_integral_grad_rays); a position carries no energy: rows 0 and 1 are written as 0 (ACCUM: left
//            alone, and rows 2 and 3 get buffer + fp32(term), added in fp32).
// PARTIAL and RAYS pick the outputs; a ray with ra = 0 contributes exactly 0.
template <bool BIG, class M, bool PARTIAL, bool RAYS, bool ACCUM>
__global__ void __launch_bounds__(kGradThreads)
k_dp_energy_grad(sdirt_rays R, int64_t S, int64_t Mtot, DevDpParams dp, DpGrad q, GradLaunch gl_,
                 const double* __restrict__ grad_e, double* __restrict__ partial, float* __restrict__ ray_grad)
{
    const Slice b = block_slice(gl_, S);
    const auto div_fmh = UDiv<M>::make(dp.fmh);
    const double g_l = grad_e[kEnergyComps * b.n], g_r = grad_e[kEnergyComps * b.n + 1];
    double acc[kEnergyComps] = {};
    for (int64_t s = b.s_begin + threadIdx.x; s < b.s_end; s += kGradThreads) {
        const int64_t i = b.n * S + s;
        const float dx = R.dx[i], dz = R.dz[i], ra = R.ra[i];
        float g_dx = 0.0f, g_dz = 0.0f;
        if (ra != 0.0f) {
            const float x_tan = (-dx) / dz;
            const double w = ra;
            if (PARTIAL) {
                double dZ[3][3];
                dz_boundaries<BIG, M>(dp, div_fmh, q, x_tan, dZ);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double dsr = dZ[1][c] - dZ[0][c], dsl = dZ[2][c] - dZ[1][c];
                    acc[c] += w * (g_l * dsl + g_r * dsr);
                }
            }
            if (RAYS) {
                double dT[3];
                dz_dt<BIG, M>(dp, div_fmh, q, x_tan, dT);
                const double dt = w * (g_l * (dT[2] - dT[1]) + g_r * (dT[1] - dT[0]));          // dLoss/d(x_tan)
                const double z = (double)dz;
                g_dx = (float)(-dt / z);
                g_dz = (float)(dt * (double)dx / (z * z));
            }
        }
        if (RAYS) {
            if (ACCUM) {
                ray_grad[2 * Mtot + i] = ray_grad[2 * Mtot + i] + g_dx;
                ray_grad[3 * Mtot + i] = ray_grad[3 * Mtot + i] + g_dz;
            } else {
                ray_grad[i] = 0.0f; ray_grad[Mtot + i] = 0.0f; ray_grad[2 * Mtot + i] = g_dx; ray_grad[3 * Mtot + i] = g_dz;
            }
        }
    }
    if (PARTIAL) block_sum_store<kEnergyComps>(acc, partial + (b.n * gl_.nslices + b.j) * kEnergyComps);
}

GradLaunch plan_grad(int64_t N, int64_t S, int ncu)
{
    GradLaunch g{};
    // about eight workgroups per CU in all, each with at least four rays per thread
    int64_t ns = std::max<int64_t>(1, (8 * (int64_t)ncu + N - 1) / std::max<int64_t>(N, 1));
    ns = std::min<int64_t>(ns, std::max<int64_t>(1, S / (4 * kGradThreads)));
    g.chunk = std::max<int64_t>(1, (S + ns - 1) / ns);
    g.nslices = (int)std::max<int64_t>(1, (S + g.chunk - 1) / g.chunk);
    return g;
}

// The argument checks and the launch plan the five entries share, in the order the statuses come out; `own` holds the
// checks of the entry that belong between the rays and the sizes.  SDIRT_OK with gl.nslices = 0 when N = 0.
template <class Own>
int check_and_plan(const sdirt_rays& rays, int64_t S, int64_t N, const sdirt_dp_params* dp, int32_t n_slices, Own&& own,
                   GradLaunch& gl)
{
    gl = GradLaunch{};
    if (int rc = check_rays(rays)) return rc;
    if (int rc = own()) return rc;
    if (S < 0 || N < 0 || N > (1ll << 30)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
    if (dp && !(dp->r > 0.0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->r must be > 0");
    if (dp && !(dp->f != dp->h)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->f must differ from dp->h");
    if (N == 0) return SDIRT_OK;
    int ncu = 0;
    if (int rc = device_cus(&ncu)) return rc;
    gl = plan_grad(N, S, ncu);
    if (n_slices != gl.nslices)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_slices=%d, the launch has %d (sdirt_forward_integral_grad_slices)",
                    n_slices, gl.nslices);
    return SDIRT_OK;
}

}  // namespace

extern "C" {

int32_t sdirt_forward_integral_grad_slices(int64_t n_points, int64_t spp, int32_t n_cus)
{
    if (n_points < 1 || spp < 0 || n_cus < 1) return 0;
    return plan_grad(n_points, spp, n_cus).nslices;
}

static int launch_integral_grad(sdirt_rays rays, int64_t S, int64_t N, double ps, int32_t ks, const float* center,
                                const sdirt_dp_params* dp, uint32_t flags, const float* grad_l, const float* grad_r,
                                double* partial, int32_t n_slices, float* ray_grad, bool focus, void* stream)
{
    GradLaunch gl;
    const auto own = [&] {
        if (int rc = check_ks(ks, SDIRT_MAX_KS_STAGED)) return rc;
        if (!center || (!partial && !ray_grad)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad argument");
        return (int)SDIRT_OK;
    };
    if (int rc = check_and_plan(rays, S, N, dp, n_slices, own, gl)) return rc;
    if (N == 0) return SDIRT_OK;
    hipStream_t st = as_stream(stream);
    const SplatGeom gm = make_geom(ps, ks);
    const DevDpParams dpp = make_dp(dp);
    const DpGrad q = make_dp_grad(dp);
    gl.dwr_dcx = -(double)gm.ksm1 / (double)gm.dx_rng;
    gl.dwb_dcy = -(double)gm.ksm1 / (double)gm.dy_rng;
    // param_list=None: the R grid is all zero, nothing flows back from it
    const float* gr = dpp.have_r ? grad_r : nullptr;
    const size_t lds = 2 * sizeof(float) * (size_t)ks * ks;
    const bool stage = lds <= (size_t)kGradLdsBytes;
    const unsigned grid = (unsigned)(N * gl.nslices);
    with_bool(dpp.big, [&](auto bg) { return with_bool(stage, [&](auto stg) { return with_math(flags, [&](auto m) {
        constexpr bool BG = decltype(bg)::value, STG = decltype(stg)::value;
        using Mm = decltype(m);
        const size_t dyn = STG ? lds : 0;
        if (partial && focus)        // [N, n_slices, 6]
            k_forward_integral_grad<BG, Mm, STG, true><<<grid, kGradThreads, dyn, st>>>(rays, S, gm, dpp, q, gl, center, grad_l, gr, partial);
        else if (partial)            // [N, n_slices, 5]
            k_forward_integral_grad<BG, Mm, STG, false><<<grid, kGradThreads, dyn, st>>>(rays, S, gm, dpp, q, gl, center, grad_l, gr, partial);
        if (ray_grad)
            k_forward_integral_grad_rays<BG, Mm, STG><<<grid, kGradThreads, dyn, st>>>(rays, S, S * N, gm, dpp, q, gl, center, grad_l, gr, ray_grad);
        return 0;
    }); }); });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_forward_integral_grad(sdirt_rays rays, int64_t S, int64_t N, double ps, int32_t ks, const float* center,
                                const sdirt_dp_params* dp, uint32_t flags, const float* grad_l, const float* grad_r,
                                double* partial, int32_t n_slices, void* stream)
{
    return launch_integral_grad(rays, S, N, ps, ks, center, dp, flags, grad_l, grad_r, partial, n_slices, nullptr, false, stream);
}

int sdirt_forward_integral_grad_focus(sdirt_rays rays, int64_t S, int64_t N, double ps, int32_t ks, const float* center,
                                      const sdirt_dp_params* dp, uint32_t flags, const float* grad_l, const float* grad_r,
                                      double* partial, int32_t n_slices, void* stream)
{
    if (!partial) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null partial");
    return launch_integral_grad(rays, S, N, ps, ks, center, dp, flags, grad_l, grad_r, partial, n_slices, nullptr, true, stream);
}

int sdirt_forward_integral_grad_rays(sdirt_rays rays, int64_t S, int64_t N, double ps, int32_t ks, const float* center,
                                     const sdirt_dp_params* dp, uint32_t flags, const float* grad_l,
                                     const float* grad_r, double* partial, int32_t n_slices, float* ray_grad,
                                     void* stream)
{
    if (!ray_grad) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null ray_grad");      // partial may be NULL: the rays' terms only
    return launch_integral_grad(rays, S, N, ps, ks, center, dp, flags, grad_l, grad_r, partial, n_slices, ray_grad, false, stream);
}

// The energy needs the dual-pixel parameters: the one check of its own both energy entries make after the rays'.
static int need_dp(const sdirt_dp_params* dp)
{
    return dp ? (int)SDIRT_OK : fail(SDIRT_ERR_INVALID_ARGUMENT, "null dp: the energy needs the dual-pixel parameters");
}

int sdirt_dp_energy(sdirt_rays rays, int64_t S, int64_t N, const sdirt_dp_params* dp, uint32_t flags, double* partial,
                    int32_t n_slices, void* stream)
{
    if (!partial) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null partial");
    GradLaunch gl;
    if (int rc = check_and_plan(rays, S, N, dp, n_slices, [&] { return need_dp(dp); }, gl)) return rc;
    if (N == 0) return SDIRT_OK;
    const DevDpParams dpp = make_dp(dp);
    const unsigned grid = (unsigned)(N * gl.nslices);
    hipStream_t st = as_stream(stream);
    with_bool(dpp.big, [&](auto bg) { return with_math(flags, [&](auto m) {
        k_dp_energy<decltype(bg)::value, decltype(m)><<<grid, kGradThreads, 0, st>>>(rays, S, dpp, gl, partial);
        return 0;
    }); });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_dp_energy_grad(sdirt_rays rays, int64_t S, int64_t N, const sdirt_dp_params* dp, uint32_t flags,
                         const double* grad_e, double* partial, int32_t n_slices, float* ray_grad, int32_t accumulate,
                         void* stream)
{
    if (!grad_e) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null grad_e");
    if (!partial && !ray_grad) return fail(SDIRT_ERR_INVALID_ARGUMENT, "partial and ray_grad are both null");
    GradLaunch gl;
    if (int rc = check_and_plan(rays, S, N, dp, n_slices, [&] { return need_dp(dp); }, gl)) return rc;
    if (N == 0) return SDIRT_OK;
    const DevDpParams dpp = make_dp(dp);
    const DpGrad q = make_dp_grad(dp);
    const unsigned grid = (unsigned)(N * gl.nslices);
    hipStream_t st = as_stream(stream);
    with_bool(dpp.big, [&](auto bg) { return with_math(flags, [&](auto m) {
        constexpr bool BG = decltype(bg)::value;
        using Mm = decltype(m);
        if (partial)
            k_dp_energy_grad<BG, Mm, true, false, false><<<grid, kGradThreads, 0, st>>>(rays, S, S * N, dpp, q, gl, grad_e, partial, nullptr);
        if (ray_grad && accumulate)
            k_dp_energy_grad<BG, Mm, false, true, true><<<grid, kGradThreads, 0, st>>>(rays, S, S * N, dpp, q, gl, grad_e, nullptr, ray_grad);
        else if (ray_grad)
            k_dp_energy_grad<BG, Mm, false, true, false><<<grid, kGradThreads, 0, st>>>(rays, S, S * N, dpp, q, gl, grad_e, nullptr, ray_grad);
        return 0;
    }); });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

}  // extern "C"
