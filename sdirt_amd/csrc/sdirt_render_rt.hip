// sdirt_render_rt.hip -- ray-traced rendering of a textured fronto-parallel plane through the lens (MI355X / gfx950
// only): the backward renderer the reference names and never defines (deeplens/optics.py:497-538 sample_sensor,
// :630-635 trace2obj, :756-780 render_single_img(method='raytracing')).  One kernel: sample a sensor-side ray, take
// its dual-pixel weights, trace it backward through every surface, carry it to the plane, read the texture, sum.
// No PSF, no window, no per-pixel normalisation of a kernel: the yardstick for the PSF renders.
// A second kernel, k_render_layers, renders a STACK of such planes, each with a coverage map, composited front to back
// along every ray: a scene with depth discontinuities, which the reference cannot render at all.
// A third, k_render_layers_grad, is that render's backward pass into the textures and the coverage maps:
// the same rays again, and a scatter of float64 atomic adds -- ADDED to its outputs, not the same bits on every run.
// A fourth, k_render_layers_dp_grad, is its backward pass into the dual-pixel parameters h, f, w: the
// same rays once more, the weights' derivative per ray (sdirt_dp_grad.hpp), one row of three sums per workgroup --
// no atomics, the same bits on every run.
// A fifth, k_render_layers_depth_grad, is its backward pass into the layer depths and the layers' texel scales
// (DESIGN.md §7s): a layer's depth enters only after the trace, so the derivative is a bilinear lookup's derivative
// times the ray's slope, pushed through §7q's compositing adjoint; one row of 2 L sums per workgroup, no atomics.
#include <hip/hip_runtime.h>

#include "../../include/sdirt_dp.h"
#include "sdirt_dp_grad.hpp"
#include "sdirt_trace.hpp"

using namespace sdirt;

namespace {

constexpr int kDpNone = 0, kDpSmall = 1, kDpBig = 2;
constexpr int kMaxPlanes = 4;          // texture planes one launch accumulates: 2 (NT + 1) doubles per lane

// Everything of a launch behind the trip table (which sits at kernel-argument offset 0, as in k_trace).
struct PlaneLaunch {
    const DevSurface* lens;
    int K;
    const float* x1;                   // [W] sensor x of the pixel columns
    const float* y1;                   // [H] sensor y of the pixel rows
    const float* x2;                   // [S, H, W] pupil points
    const float* y2;
    float z_sensor, z_pupil, depth, inv_texel;
    int S, H, W;
    const float* tex;                  // the first plane of this launch, [NT, Ht, Wt]
    int Ht, Wt;
    int64_t view_stride;               // elements between the views of num: n_tex H W
    double* num;                       // this launch's first plane of view 0
    double* den;                       // [V, H, W]
    float* landing;                    // [5, S, H, W] or null
    uint32_t* conv_mask;               // [K] or null
};

// floor(a) as a texel index clamped to [0, n - 1] (replicate addressing).  A NaN -- the landing point of a dead ray, which
// contributes nothing -- goes to texel 0: fmaxf returns its other operand, so nothing out of range is ever converted.
__device__ __forceinline__ int clamped_texel(float fl, int off, int n)
{
    const float c = __builtin_fminf(__builtin_fmaxf(fl, -2.0f), (float)n);
    const int i = (int)c + off;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// A lane owns a pixel, a wave 64 consecutive pixels of the row-major sensor, and walks that pixel's samples in order:
// the [S, H, W] pupil arrays are read as contiguous 256-byte runs, the 2 (NT + 1) float64 sums of a pixel stay in the
// lane's registers and are written once (OVERWRITTEN: a wrong bet on the trip table launches the call again), and
// the summation order is the sample order -- the same bits every run.
template <class M, int DP, int NT>
__global__ void __launch_bounds__(kBlock)
k_render_plane(TripTable trips /* kernarg offset 0 */, PlaneLaunch a, DevDpParams dp)
{
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
    __syncthreads();
    constexpr int V = DP == kDpNone ? 1 : 2;
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p < HW) {
        const int i = (int)(p / a.W), j = (int)(p - (int64_t)i * a.W);
        const float ox = a.x1[j], oy = a.y1[i];
        const float half_w = (float)a.Wt * 0.5f, half_h = (float)a.Ht * 0.5f;
        const int64_t plane = (int64_t)a.Ht * a.Wt;
        const auto div_fmh = UDiv<M>::make(dp.fmh);
        double num[V][NT] = {}, den[V] = {};
        for (int s = 0; s < a.S; ++s) {
            const int64_t q = (int64_t)s * HW + p;
            Ray r = make_ray<M>(ox, oy, a.z_sensor, a.x2[q], a.y2[q], a.z_pupil);
            // monte_carlo.py:48 on the ray as it ARRIVES at the sensor (direction -d), the staged splat's division.
            // The image is indexed by SENSOR position, psf_lr's grids by its negative (monte_carlo.py:24 flips the
            // points): what the splat's sl-weighted rays form is, column for column, psf_lr's L turned by 180 degrees.
            // The lens and the sub-pixel model are symmetric under that turn with the two sub-pixels exchanged, so
            // the view that shifts with defocus as psf_lr's L does is the sr-weighted one: (w_L, w_R) = (sr, sl).
            float w[2] = {1.0f, 1.0f};
            if (DP != kDpNone) {
                const float x_tan = r.dx / (-r.dz);
                if (DP == kDpBig) dp_weights_big(dp, x_tan, w[1], w[0]);
                else dp_weights_small<M>(dp, div_fmh, x_tan, w[1], w[0]);
            }
            trace_ray<false, M, true, /*UNIT_W*/ true, /*MASKS*/ true>(a.lens, 0, a.K, kernarg_at(0), r, lds_mask);
            propagate_to<Ieee>(r, a.depth);                       // k_propagate's arithmetic
            if (a.landing) {
                const int64_t M5 = (int64_t)a.S * HW;
                a.landing[q] = r.ox; a.landing[M5 + q] = r.oy; a.landing[2 * M5 + q] = r.ra;
                a.landing[3 * M5 + q] = w[0]; a.landing[4 * M5 + q] = DP != kDpNone ? w[1] : 1.0f;
            }
            if (!(r.ra != 0.0f)) continue;
            // the lookup of DESIGN.md §7o, one rounding per operation
            const float u = half_w - r.ox * a.inv_texel, v = half_h + r.oy * a.inv_texel;
            const float ta = u - 0.5f, tb = v - 0.5f;
            const float c0 = __builtin_floorf(ta), r0 = __builtin_floorf(tb);
            const float fu = ta - c0, fv = tb - r0;
            const int cl = clamped_texel(c0, 0, a.Wt), cr = clamped_texel(c0, 1, a.Wt);
            const int rt = clamped_texel(r0, 0, a.Ht), rb = clamped_texel(r0, 1, a.Ht);
            const double du = fu, dv = fv;
            const double w00 = (1.0 - dv) * (1.0 - du), w01 = (1.0 - dv) * du, w10 = dv * (1.0 - du), w11 = dv * du;
            double wr[V];
#pragma unroll
            for (int side = 0; side < V; ++side) {
                wr[side] = (double)w[side] * (double)r.ra;
                den[side] += wr[side];
            }
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const float* __restrict__ t = a.tex + k * plane;
                const double t00 = t[rt * a.Wt + cl], t01 = t[rt * a.Wt + cr], t10 = t[rb * a.Wt + cl], t11 = t[rb * a.Wt + cr];
                const double tk = w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11;
#pragma unroll
                for (int side = 0; side < V; ++side) num[side][k] += wr[side] * tk;
            }
        }
#pragma unroll
        for (int side = 0; side < V; ++side) {
            a.den[side * HW + p] = den[side];
#pragma unroll
            for (int k = 0; k < NT; ++k) a.num[side * a.view_stride + k * HW + p] = num[side][k];
        }
    }
    __syncthreads();
    if (a.conv_mask && (int)threadIdx.x < a.K && lds_mask[threadIdx.x])
        atomicOr(&a.conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

// One instantiation per (math policy, dual-pixel form, planes per launch).
template <class M, int DP>
int launch_planes(int nt, dim3 grid, hipStream_t st, const TripTable& tt, const PlaneLaunch& a, const DevDpParams& dp)
{
    switch (nt) {
    case 1: k_render_plane<M, DP, 1><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    case 2: k_render_plane<M, DP, 2><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    case 3: k_render_plane<M, DP, 3><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    default: k_render_plane<M, DP, kMaxPlanes><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    }
    return 0;
}

// ---- a stack of planes with coverage, composited front to back along every ray ----------------------

// Everything of a layered launch behind the trip table.  depth and inv_texel of every layer travel here, in the kernel
// arguments: the layer index is wave-uniform, so they arrive through scalar loads and need no table on the device.
struct LayersLaunch {
    const DevSurface* lens;
    int K;
    const float* x1;
    const float* y1;
    const float* x2;
    const float* y2;
    float z_sensor, z_pupil;
    int S, H, W, L;
    float depth[SDIRT_MAX_LAYERS];     // 0 > depth[0] > depth[1] > ...: layer 0 is met first by a backward ray
    float inv_texel[SDIRT_MAX_LAYERS];
    const float* alpha;                // [L, Ht, Wt]
    const float* tex;                  // the first plane of this launch in layer 0
    int64_t layer_stride;              // elements between the layers of tex; 0: one [NT, Ht, Wt] shared by all
    int Ht, Wt;
    int64_t view_stride;
    double* num;
    double* den;                       // [V, H, W]
    double* cov;                       // [V, H, W]
    float* landing;                    // [3 + 2 L, S, H, W] or null
    uint32_t* conv_mask;
};

// The lookup of DESIGN.md §7o at a landing point, one rounding per operation (k_render_plane's statements, which
// tools/variants/rt_*.py edit by their text, stay where they are): the four taps' offsets in a plane under replicate
// addressing and their float64 weights.  A layer reads its coverage and each of its colour planes through one of these.
struct Taps {
    int i00, i01, i10, i11;
    double w00, w01, w10, w11;
    __device__ __forceinline__ Taps(float px, float py, float inv_texel, int Ht, int Wt)
    {
        const float half_w = (float)Wt * 0.5f, half_h = (float)Ht * 0.5f;
        const float u = half_w - px * inv_texel, v = half_h + py * inv_texel;
        const float ta = u - 0.5f, tb = v - 0.5f;
        const float c0 = __builtin_floorf(ta), r0 = __builtin_floorf(tb);
        const float fu = ta - c0, fv = tb - r0;
        const int cl = clamped_texel(c0, 0, Wt), cr = clamped_texel(c0, 1, Wt);
        const int rt = clamped_texel(r0, 0, Ht), rb = clamped_texel(r0, 1, Ht);
        i00 = rt * Wt + cl; i01 = rt * Wt + cr; i10 = rb * Wt + cl; i11 = rb * Wt + cr;
        const double du = fu, dv = fv;
        w00 = (1.0 - dv) * (1.0 - du); w01 = (1.0 - dv) * du; w10 = dv * (1.0 - du); w11 = dv * du;
    }
    __device__ __forceinline__ double read(const float* __restrict__ t) const
    {
        const double t00 = t[i00], t01 = t[i01], t10 = t[i10], t11 = t[i11];
        return w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11;
    }
};

// k_render_plane's geometry and per-ray program up to the end of the trace.  Then every layer's landing point is
// propagate_to<Ieee> on a COPY of the ray as the trace left it (never chained from layer to layer: each equals
// k_render_plane's landing at that depth in every bit), and the ray's colour c_k and transmittance T are composited in
// float64 in the order of DESIGN.md §7p.  A lane whose T has reached 0 skips the lookups of the layers behind (with
// finite textures they add exact zeros); their landing points are still written when a record is asked for.
template <class M, int DP, int NT>
__global__ void __launch_bounds__(kBlock)
k_render_layers(TripTable trips /* kernarg offset 0 */, LayersLaunch a, DevDpParams dp)
{
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
    __syncthreads();
    constexpr int V = DP == kDpNone ? 1 : 2;
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p < HW) {
        const int i = (int)(p / a.W), j = (int)(p - (int64_t)i * a.W);
        const float ox = a.x1[j], oy = a.y1[i];
        const int64_t plane = (int64_t)a.Ht * a.Wt;
        const int64_t rows = (int64_t)a.S * HW;
        const auto div_fmh = UDiv<M>::make(dp.fmh);
        double num[V][NT] = {}, den[V] = {}, cov[V] = {};
        for (int s = 0; s < a.S; ++s) {
            const int64_t q = (int64_t)s * HW + p;
            Ray r = make_ray<M>(ox, oy, a.z_sensor, a.x2[q], a.y2[q], a.z_pupil);
            float wv[2] = {1.0f, 1.0f};                        // the views' weights (w_L, w_R) = (sr, sl): see k_render_plane
            if (DP != kDpNone) {
                const float x_tan = r.dx / (-r.dz);
                if (DP == kDpBig) dp_weights_big(dp, x_tan, wv[1], wv[0]);
                else dp_weights_small<M>(dp, div_fmh, x_tan, wv[1], wv[0]);
            }
            trace_ray<false, M, true, /*UNIT_W*/ true, /*MASKS*/ true>(a.lens, 0, a.K, kernarg_at(0), r, lds_mask);
            if (a.landing) {
                a.landing[q] = r.ra; a.landing[rows + q] = wv[0]; a.landing[2 * rows + q] = DP != kDpNone ? wv[1] : 1.0f;
            }
            const bool live = r.ra != 0.0f;
            double T = 1.0, c[NT] = {};
            for (int l = 0; l < a.L; ++l) {
                const bool reads = live && T != 0.0;
                if (!reads && !a.landing) break;
                Ray at = r;
                propagate_to<Ieee>(at, a.depth[l]);
                if (a.landing) {
                    a.landing[(3 + 2 * l) * rows + q] = at.ox; a.landing[(4 + 2 * l) * rows + q] = at.oy;
                }
                if (!reads) continue;
                const Taps taps(at.ox, at.oy, a.inv_texel[l], a.Ht, a.Wt);
                const double al = taps.read(a.alpha + l * plane);
                const double g = T * al;
                const float* __restrict__ tl = a.tex + l * a.layer_stride;
#pragma unroll
                for (int k = 0; k < NT; ++k) c[k] = c[k] + g * taps.read(tl + k * plane);
                T = T * (1.0 - al);
            }
            if (!live) continue;
            const double o = 1.0 - T;
#pragma unroll
            for (int side = 0; side < V; ++side) {
                const double wr = (double)wv[side] * (double)r.ra;
                den[side] += wr;
                cov[side] += wr * o;
#pragma unroll
                for (int k = 0; k < NT; ++k) num[side][k] += wr * c[k];
            }
        }
#pragma unroll
        for (int side = 0; side < V; ++side) {
            a.den[side * HW + p] = den[side];
            a.cov[side * HW + p] = cov[side];
#pragma unroll
            for (int k = 0; k < NT; ++k) a.num[side * a.view_stride + k * HW + p] = num[side][k];
        }
    }
    __syncthreads();
    if (a.conv_mask && (int)threadIdx.x < a.K && lds_mask[threadIdx.x])
        atomicOr(&a.conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

template <class M, int DP>
int launch_layers(int nt, dim3 grid, hipStream_t st, const TripTable& tt, const LayersLaunch& a, const DevDpParams& dp)
{
    switch (nt) {
    case 1: k_render_layers<M, DP, 1><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    case 2: k_render_layers<M, DP, 2><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    case 3: k_render_layers<M, DP, 3><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    default: k_render_layers<M, DP, kMaxPlanes><<<grid, kBlock, 0, st>>>(tt, a, dp); break;
    }
    return 0;
}

// ---- the layered render's backward: a scatter into the textures and the coverage maps ---------------

// Everything of a backward launch behind the trip table.  (Named b in the kernel, its layers m, its weights ws: the
// statements of the two forward kernels, which tools/variants/rt_*.py and rl_*.py find by their text, stay unique.)
struct LayersGradLaunch {
    const DevSurface* lens;
    int K;
    const float* x1;
    const float* y1;
    const float* x2;
    const float* y2;
    float z_sensor, z_pupil;
    int S, H, W, L;
    float depth[SDIRT_MAX_LAYERS];
    float inv_texel[SDIRT_MAX_LAYERS];
    const float* alpha;                // [L, Ht, Wt], or null: every layer opaque
    const float* tex;                  // the first plane of this launch in layer 0
    int64_t layer_stride;
    int Ht, Wt;
    int64_t view_stride;               // elements between the views of gnum: n_tex H W
    const double* gnum;                // this launch's first plane of view 0
    double* galpha;                    // [L, Ht, Wt] or null, ADDED to
    double* gtex;                      // this launch's first plane in layer 0, or null, ADDED to
    int64_t gtex_layer_stride;         // elements between the layers of gtex; 0: one [NT, Ht, Wt] all layers add into
};

// The four adds of one lookup's adjoint: v w_j into each tap.  Under replicate addressing two taps can be one texel;
// both adds go to it.  One global_atomic_add_f64 each (docs/KERNEL_NOTES.md), no return value, no loop.
__device__ __forceinline__ void scatter_taps(double* __restrict__ g, const Taps& tp, double v)
{
    atomicAdd(g + tp.i00, v * tp.w00);
    atomicAdd(g + tp.i01, v * tp.w01);
    atomicAdd(g + tp.i10, v * tp.w10);
    atomicAdd(g + tp.i11, v * tp.w11);
}

// k_render_layers' geometry and per-ray program up to the end of the trace, with the trip table the forward ended
// with (no convergence masks: that table is the one the forward verified), so every landing point, ra and weight is
// the forward's in every bit.  Then two walks over the layers of a live ray, all in float64, one rounding per
// operation, in the order of DESIGN.md §7q:
//   front to back over ALL layers -- also those behind T == 0, which the forward never read: the coverage gradient of
//   the texel that stopped the ray depends on them -- D_m = sum_k q_k t_{m,k} and T_m go to a lane-major LDS stash
//   [L][2][kBlock] (a register array indexed by m would go to scratch), and the colour adjoint (q_k g_m) w_j is added;
//   back to front: d = D_m - R, (T_m d) w_j is added to the coverage gradient, R = R + a_m d.  The taps and a_m are
//   formed again there (the same fp32 steps on the same ray: the same bits; four cached loads) instead of being stashed:
//   two doubles per layer and lane keep 16 layers within 64 KB of LDS.
// Terms whose factor T_m (colour: g_m) is 0 are exact zeros and are not issued.  Without a coverage gradient the
// front-to-back walk ends where T reaches 0, as the forward's does, and nothing is stashed.
// The outputs are ADDED to with float64 atomics: the sums depend on the order the adds arrive in, so two runs need
// NOT agree in every bit (they agree within the summation bound of §7q).  Everything else here is deterministic.
template <class M, int DP, int NT>
__global__ void __launch_bounds__(kBlock)
k_render_layers_grad(TripTable trips /* kernarg offset 0 */, LayersGradLaunch b, DevDpParams dp)
{
    extern __shared__ double stash[];                          // [L][2][kBlock]: D_m, T_m of this lane's ray
    constexpr int V = DP == kDpNone ? 1 : 2;
    const int64_t HW = (int64_t)b.H * b.W;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int i = (int)(p / b.W), j = (int)(p - (int64_t)i * b.W);
    const float ox = b.x1[j], oy = b.y1[i];
    const int64_t plane = (int64_t)b.Ht * b.Wt;
    const auto div_fmh = UDiv<M>::make(dp.fmh);
    double* const mine = stash + threadIdx.x;
    double gn[V][NT];
#pragma unroll
    for (int side = 0; side < V; ++side)
#pragma unroll
        for (int k = 0; k < NT; ++k) gn[side][k] = b.gnum[side * b.view_stride + k * HW + p];
    for (int s = 0; s < b.S; ++s) {
        const int64_t q = (int64_t)s * HW + p;
        Ray r = make_ray<M>(ox, oy, b.z_sensor, b.x2[q], b.y2[q], b.z_pupil);
        float ws[2] = {1.0f, 1.0f};                            // (w_L, w_R) = (sr, sl): see k_render_plane
        if (DP != kDpNone) {
            const float x_tan = r.dx / (-r.dz);
            if (DP == kDpBig) dp_weights_big(dp, x_tan, ws[1], ws[0]);
            else dp_weights_small<M>(dp, div_fmh, x_tan, ws[1], ws[0]);
        }
        trace_ray<false, M, true, /*UNIT_W*/ true, /*MASKS*/ false>(b.lens, 0, b.K, kernarg_at(0), r, nullptr);
        if (!(r.ra != 0.0f)) continue;
        double qk[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            qk[k] = ((double)ws[0] * (double)r.ra) * gn[0][k];
            if (V == 2) qk[k] = qk[k] + ((double)ws[1] * (double)r.ra) * gn[V - 1][k];
        }
        double Tm = 1.0;
        int walked = 0;                                        // layers the first walk visited
        for (int m = 0; m < b.L; ++m) {
            if (!b.galpha && Tm == 0.0) break;
            Ray hit = r;
            propagate_to<Ieee>(hit, b.depth[m]);
            const Taps tp(hit.ox, hit.oy, b.inv_texel[m], b.Ht, b.Wt);
            const double cover = b.alpha ? tp.read(b.alpha + m * plane) : 1.0;
            const double gm = Tm * cover;
            if (b.galpha) {
                const float* __restrict__ tm = b.tex + m * b.layer_stride;
                double D = 0.0;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const double term = qk[k] * tp.read(tm + k * plane);
                    D = k == 0 ? term : D + term;
                }
                mine[(2 * m) * kBlock] = D;
                mine[(2 * m + 1) * kBlock] = Tm;
            }
            if (b.gtex && gm != 0.0) {
                double* __restrict__ gt = b.gtex + m * b.gtex_layer_stride;
#pragma unroll
                for (int k = 0; k < NT; ++k) scatter_taps(gt + k * plane, tp, qk[k] * gm);
            }
            Tm = Tm * (1.0 - cover);
            walked = m + 1;
        }
        if (!b.galpha) continue;
        double R = 0.0;
        for (int m = walked - 1; m >= 0; --m) {
            const double D = mine[(2 * m) * kBlock], Tb = mine[(2 * m + 1) * kBlock];
            Ray hit = r;
            propagate_to<Ieee>(hit, b.depth[m]);
            const Taps tp(hit.ox, hit.oy, b.inv_texel[m], b.Ht, b.Wt);
            const double cover = tp.read(b.alpha + m * plane);
            const double d = D - R;
            if (Tb != 0.0) scatter_taps(b.galpha + m * plane, tp, Tb * d);
            R = R + cover * d;
        }
    }
}

template <class M, int DP>
int launch_layers_grad(int nt, dim3 grid, size_t lds, hipStream_t st, const TripTable& tt, const LayersGradLaunch& b,
                       const DevDpParams& dp)
{
    switch (nt) {
    case 1: k_render_layers_grad<M, DP, 1><<<grid, kBlock, lds, st>>>(tt, b, dp); break;
    case 2: k_render_layers_grad<M, DP, 2><<<grid, kBlock, lds, st>>>(tt, b, dp); break;
    case 3: k_render_layers_grad<M, DP, 3><<<grid, kBlock, lds, st>>>(tt, b, dp); break;
    default: k_render_layers_grad<M, DP, kMaxPlanes><<<grid, kBlock, lds, st>>>(tt, b, dp); break;
    }
    return 0;
}

// ---- the layered render's backward into the dual-pixel parameters h, f, w ---------------------------

static_assert(kBlock == kGradThreads, "block_sum_store reduces a workgroup of kGradThreads");

// Everything of a dual-pixel backward launch behind the trip table.  (Named e in the kernel, its layers n, its ray at
// a layer `met`: the statements of the three kernels above, which tools/variants/*.py find by their text, stay unique.
// There is no weight array: the adjoint needs the weights' derivative, not the weights.)
struct LayersDpGradLaunch {
    const DevSurface* lens;
    int K;
    const float* x1;
    const float* y1;
    const float* x2;
    const float* y2;
    float z_sensor, z_pupil;
    int S, H, W, L;
    float depth[SDIRT_MAX_LAYERS];
    float inv_texel[SDIRT_MAX_LAYERS];
    const float* alpha;                // [L, Ht, Wt], or null: every layer opaque
    const float* tex;                  // the first plane of this launch in layer 0
    int64_t layer_stride;
    int Ht, Wt;
    int64_t view_stride;               // elements between the views of gnum: n_tex H W
    const double* gnum;                // this launch's first plane of view 0
    const double* gden;                // [2, H, W], or null: no adjoint of den (photometric; a plane group past the first)
    double* partial;                   // this launch's [ceil(H W / kBlock), 3], OVERWRITTEN
    float* x_tan;                      // [S, H, W] or null
};

// k_render_layers_grad's geometry and per-ray program up to the end of the trace, with the trip table the forward
// ended with, so x_tan, ra and every landing point are the forward's in every bit.  Then, for a live ray, the
// forward's walk over the layers (it ends where T reaches 0) gives the composite c_k, and
//   A_side = ra (gnum[side, 0] c_0 + ... + gnum[side, NT-1] c_{NT-1} + gden[side])
// is what the ray's weight w_side is multiplied by in the loss.  The weights' derivative in h, f, w (dz_boundaries: the
// float64 chords on the forward's fp32 clamp decisions) is evaluated AFTER the trace and only where A_0, A_1 are not
// both 0: six float64 square roots and a division chain that dead rays, and pixels no adjoint reaches, never pay for,
// and whose registers are not live across the surface loop (x_tan alone is carried over it).
// A lane adds its rays' terms in sample order; the workgroup's sum (wave_sum, block_sum_store<3>) is one row of
// `partial`, OVERWRITTEN.  Lanes past H W take part with zeros.  No atomics: the same bits on every run.
template <class M, int DP, int NT>
__global__ void __launch_bounds__(kBlock)
k_render_layers_dp_grad(TripTable trips /* kernarg offset 0 */, LayersDpGradLaunch e, DevDpParams dp, DpGrad q)
{
    const int64_t HW = (int64_t)e.H * e.W;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc[3] = {};
    if (p < HW) {
        const int i = (int)(p / e.W), j = (int)(p - (int64_t)i * e.W);
        const float ox = e.x1[j], oy = e.y1[i];
        const int64_t plane = (int64_t)e.Ht * e.Wt;
        const auto div_fmh = UDiv<M>::make(dp.fmh);
        double gn[2][NT], gd[2];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            gd[side] = e.gden ? e.gden[side * HW + p] : 0.0;
#pragma unroll
            for (int k = 0; k < NT; ++k) gn[side][k] = e.gnum[side * e.view_stride + k * HW + p];
        }
        for (int s = 0; s < e.S; ++s) {
            const int64_t at_q = (int64_t)s * HW + p;
            Ray r = make_ray<M>(ox, oy, e.z_sensor, e.x2[at_q], e.y2[at_q], e.z_pupil);
            const float x_tan = r.dx / (-r.dz);                // what the forward's dp_weights_* call reads
            if (e.x_tan) e.x_tan[at_q] = x_tan;
            trace_ray<false, M, true, /*UNIT_W*/ true, /*MASKS*/ false>(e.lens, 0, e.K, kernarg_at(0), r, nullptr);
            const bool dead = !(r.ra != 0.0f);
            if (dead) continue;
            double Tn = 1.0, cn[NT] = {};
            for (int n = 0; n < e.L; ++n) {
                if (Tn == 0.0) break;
                Ray met = r;
                propagate_to<Ieee>(met, e.depth[n]);
                const Taps tq(met.ox, met.oy, e.inv_texel[n], e.Ht, e.Wt);
                const double cover = e.alpha ? tq.read(e.alpha + n * plane) : 1.0;
                const double share = Tn * cover;
                const float* __restrict__ tn = e.tex + n * e.layer_stride;
#pragma unroll
                for (int k = 0; k < NT; ++k) cn[k] = cn[k] + share * tq.read(tn + k * plane);
                Tn = Tn * (1.0 - cover);
            }
            double A[2];
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                double sum = gn[side][0] * cn[0];
#pragma unroll
                for (int k = 1; k < NT; ++k) sum = sum + gn[side][k] * cn[k];
                A[side] = (double)r.ra * (sum + gd[side]);
            }
            if (A[0] == 0.0 && A[1] == 0.0) continue;
            double dZ[3][3];
            dz_boundaries<DP == kDpBig, M>(dp, div_fmh, q, x_tan, dZ);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double dwl = dZ[1][c] - dZ[0][c], dwr = dZ[2][c] - dZ[1][c];      // (w_L, w_R) = (s_r, s_l)
                acc[c] += A[0] * dwl + A[1] * dwr;
            }
        }
    }
    block_sum_store<3>(acc, e.partial + (int64_t)blockIdx.x * 3);
}

template <class M, int DP>
int launch_layers_dp_grad(int nt, dim3 grid, hipStream_t st, const TripTable& tt, const LayersDpGradLaunch& e,
                          const DevDpParams& dp, const DpGrad& q)
{
    switch (nt) {
    case 1: k_render_layers_dp_grad<M, DP, 1><<<grid, kBlock, 0, st>>>(tt, e, dp, q); break;
    case 2: k_render_layers_dp_grad<M, DP, 2><<<grid, kBlock, 0, st>>>(tt, e, dp, q); break;
    case 3: k_render_layers_dp_grad<M, DP, 3><<<grid, kBlock, 0, st>>>(tt, e, dp, q); break;
    default: k_render_layers_dp_grad<M, DP, kMaxPlanes><<<grid, kBlock, 0, st>>>(tt, e, dp, q); break;
    }
    return 0;
}

// ---- the layered render's backward into the layer depths and texel scales ---------------------------

// Everything of a depth backward launch behind the trip table.  (Named z in the kernel, its layers `lay`, its ray at a
// layer `there`, its weights wz: the statements of the four kernels above, which tools/variants/*.py find by their
// text, stay unique.)
struct LayersDepthGradLaunch {
    const DevSurface* lens;
    int K;
    const float* x1;
    const float* y1;
    const float* x2;
    const float* y2;
    float z_sensor, z_pupil;
    int S, H, W, L;
    float depth[SDIRT_MAX_LAYERS];
    float inv_texel[SDIRT_MAX_LAYERS];
    const float* alpha;                // [L, Ht, Wt], or null: every layer opaque
    const float* tex;                  // the first plane of this launch in layer 0
    int64_t layer_stride;
    int Ht, Wt;
    int64_t view_stride;               // elements between the views of gnum: n_tex H W
    const double* gnum;                // this launch's first plane of view 0
    double* partial;                   // this launch's [ceil(H W / kBlock), L, 2], OVERWRITTEN
    float* ray_dir;                    // [3, S, H, W] or null
};

// Taps with the lookup's two fractions kept: what the derivative of a lookup in (fu, fv) is made of.  fu, fv are formed
// by Taps' own fp32 statements on the same arguments (the same bits; the compiler folds the two copies into one), so
// the floor decisions are the forward's.
struct SlopeTaps {
    Taps at;
    double du, dv;
    __device__ __forceinline__ SlopeTaps(float px, float py, float inv_texel, int Ht, int Wt)
        : at(px, py, inv_texel, Ht, Wt)
    {
        const float half_w = (float)Wt * 0.5f, half_h = (float)Ht * 0.5f;
        const float u = half_w - px * inv_texel, v = half_h + py * inv_texel;
        const float ta = u - 0.5f, tb = v - 0.5f;
        du = ta - __builtin_floorf(ta); dv = tb - __builtin_floorf(tb);
    }
    // d(read)/dfu and d(read)/dfv from the four taps the read takes.  Two taps that replicate addressing puts on one
    // texel differ by an exact 0: the derivative of the clamped lookup outside the texture and on a 1-texel extent.
    __device__ __forceinline__ void slopes(const float* __restrict__ t, double& dfu, double& dfv) const
    {
        const double v00 = t[at.i00], v01 = t[at.i01], v10 = t[at.i10], v11 = t[at.i11];
        dfu = (1.0 - dv) * (v01 - v00) + dv * (v11 - v10);
        dfv = (1.0 - du) * (v10 - v00) + du * (v11 - v01);
    }
};

// block_sum_store of sdirt_dp_grad.hpp for a run-time number of components that sit lane-major in LDS
// (mine[c * kBlock] is this thread's component c): the wave by shuffles, the waves 0 to 3 through LDS, the same fixed
// tree.  Called by all threads of the workgroup.
__device__ __forceinline__ void block_sum_store_rows(const double* mine, int comps, double* __restrict__ out)
{
    __shared__ double red_rows[kBlock / 64][2 * SDIRT_MAX_LAYERS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < comps; ++c) {
        const double v = wave_sum(mine[c * kBlock]);
        if (lane == 0) red_rows[wave][c] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < comps) {
        double v = 0.0;
        for (int k = 0; k < kBlock / 64; ++k) v += red_rows[k][threadIdx.x];
        out[threadIdx.x] = v;
    }
}

// k_render_layers_grad's geometry and per-ray program up to the end of the trace, with the trip table the forward
// ended with, so the ray the trace leaves, ra, the weights and every landing point are the forward's in every bit.
// No z_l enters before that point: the landing on layer l is px_l = ox + dx (z_l - oz) / dz, whose slope in z_l is
// sx = dx / dz, and u = Wt/2 - px_l inv_l, v = Ht/2 + py_l inv_l.  For a live ray, all in float64, one rounding per
// operation, in the order of DESIGN.md §7s:
//   front to back over ALL layers: D_l = sum_k q_k t_{l,k} and T_l go to the lane's stash (§7q's first walk without
//   its scatter);
//   back to front: d = D_l - R, e = T_l d, g = T_l a_l, Pu = e da/dfu + g sum_k q_k dt_k/dfu (Pv alike), and
//     gz_l   = inv_l (Pv sy - Pu sx)       the term of depth[l]
//     ginv_l = Pv py_l - Pu px_l           the term of inv_texel[l]
//   are added to the lane's two sums of layer l; R = R + a_l d.  Layers with T_l == 0 give exact zeros: not issued.
// With a null alpha (every layer opaque) the ray meets layer 0 with a = 1 and T = 0 behind it: one layer, no stash,
// Pu = sum_k q_k dt_k/dfu, and what lies behind is not read.
// The lane's 2 L sums and its 2 L stash entries are indexed by a run-time layer: register arrays would go to scratch,
// so both sit lane-major in dynamic LDS, [2 L][kBlock] sums and then [2 L][kBlock] stash (8 KB per layer, 128 KB at
// L = 16; the stash is left out with a null alpha).  A lane adds its rays' terms in sample order; the workgroup's sum
// is one row of `partial`, OVERWRITTEN.  Lanes past H W take part with zeros.  No atomics: the same bits on every run.
template <class M, int DP, int NT>
__global__ void __launch_bounds__(kBlock)
k_render_layers_depth_grad(TripTable trips /* kernarg offset 0 */, LayersDepthGradLaunch z, DevDpParams dp)
{
    extern __shared__ double slab[];                           // [2 L][kBlock] sums, [2 L][kBlock] stash
    constexpr int V = DP == kDpNone ? 1 : 2;
    const int64_t HW = (int64_t)z.H * z.W;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double* const sums = slab + threadIdx.x;
    double* const kept = slab + 2 * z.L * kBlock + threadIdx.x;
    for (int c = 0; c < 2 * z.L; ++c) sums[c * kBlock] = 0.0;
    if (p < HW) {
        const int i = (int)(p / z.W), j = (int)(p - (int64_t)i * z.W);
        const float ox = z.x1[j], oy = z.y1[i];
        const int64_t plane = (int64_t)z.Ht * z.Wt;
        const int64_t rays = (int64_t)z.S * HW;
        const auto div_fmh = UDiv<M>::make(dp.fmh);
        double gz[V][NT];
#pragma unroll
        for (int side = 0; side < V; ++side)
#pragma unroll
            for (int k = 0; k < NT; ++k) gz[side][k] = z.gnum[side * z.view_stride + k * HW + p];
        for (int s = 0; s < z.S; ++s) {
            const int64_t at_ray = (int64_t)s * HW + p;
            Ray r = make_ray<M>(ox, oy, z.z_sensor, z.x2[at_ray], z.y2[at_ray], z.z_pupil);
            float wz[2] = {1.0f, 1.0f};                        // (w_L, w_R) = (sr, sl): see k_render_plane
            if (DP != kDpNone) {
                const float x_tan = r.dx / (-r.dz);
                if (DP == kDpBig) dp_weights_big(dp, x_tan, wz[1], wz[0]);
                else dp_weights_small<M>(dp, div_fmh, x_tan, wz[1], wz[0]);
            }
            trace_ray<false, M, true, /*UNIT_W*/ true, /*MASKS*/ false>(z.lens, 0, z.K, kernarg_at(0), r, nullptr);
            if (z.ray_dir) {
                z.ray_dir[at_ray] = r.dx; z.ray_dir[rays + at_ray] = r.dy; z.ray_dir[2 * rays + at_ray] = r.dz;
            }
            const bool lives = r.ra != 0.0f;
            if (!lives) continue;
            const double sx = (double)r.dx / (double)r.dz, sy = (double)r.dy / (double)r.dz;
            double qz[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                qz[k] = ((double)wz[0] * (double)r.ra) * gz[0][k];
                if (V == 2) qz[k] = qz[k] + ((double)wz[1] * (double)r.ra) * gz[V - 1][k];
            }
            if (!z.alpha) {
                Ray there = r;
                propagate_to<Ieee>(there, z.depth[0]);
                const SlopeTaps st(there.ox, there.oy, z.inv_texel[0], z.Ht, z.Wt);
                double Pu = 0.0, Pv = 0.0;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    double tu, tv;
                    st.slopes(z.tex + k * plane, tu, tv);
                    Pu = k == 0 ? qz[k] * tu : Pu + qz[k] * tu;
                    Pv = k == 0 ? qz[k] * tv : Pv + qz[k] * tv;
                }
                sums[0] += (double)z.inv_texel[0] * (Pv * sy - Pu * sx);
                sums[kBlock] += Pv * (double)there.oy - Pu * (double)there.ox;
                continue;
            }
            double Tz = 1.0;
            for (int lay = 0; lay < z.L; ++lay) {
                Ray there = r;
                propagate_to<Ieee>(there, z.depth[lay]);
                const Taps tz(there.ox, there.oy, z.inv_texel[lay], z.Ht, z.Wt);
                const double cover = tz.read(z.alpha + lay * plane);
                const float* __restrict__ tl = z.tex + lay * z.layer_stride;
                double D = 0.0;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const double term = qz[k] * tz.read(tl + k * plane);
                    D = k == 0 ? term : D + term;
                }
                kept[(2 * lay) * kBlock] = D;
                kept[(2 * lay + 1) * kBlock] = Tz;
                Tz = Tz * (1.0 - cover);
            }
            double R = 0.0;
            for (int lay = z.L - 1; lay >= 0; --lay) {
                const double D = kept[(2 * lay) * kBlock], Tl = kept[(2 * lay + 1) * kBlock];
                Ray there = r;
                propagate_to<Ieee>(there, z.depth[lay]);
                const SlopeTaps st(there.ox, there.oy, z.inv_texel[lay], z.Ht, z.Wt);
                const double cover = st.at.read(z.alpha + lay * plane);
                const double d = D - R;
                if (Tl != 0.0) {
                    double au, av;
                    st.slopes(z.alpha + lay * plane, au, av);
                    const float* __restrict__ tl = z.tex + lay * z.layer_stride;
                    double Cu = 0.0, Cv = 0.0;
#pragma unroll
                    for (int k = 0; k < NT; ++k) {
                        double tu, tv;
                        st.slopes(tl + k * plane, tu, tv);
                        Cu = k == 0 ? qz[k] * tu : Cu + qz[k] * tu;
                        Cv = k == 0 ? qz[k] * tv : Cv + qz[k] * tv;
                    }
                    const double el = Tl * d, gl = Tl * cover;
                    const double Pu = el * au + gl * Cu, Pv = el * av + gl * Cv;
                    sums[(2 * lay) * kBlock] += (double)z.inv_texel[lay] * (Pv * sy - Pu * sx);
                    sums[(2 * lay + 1) * kBlock] += Pv * (double)there.oy - Pu * (double)there.ox;
                }
                R = R + cover * d;
            }
        }
    }
    block_sum_store_rows(sums, 2 * z.L, z.partial + (int64_t)blockIdx.x * 2 * z.L);
}

template <class M, int DP, int NT>
int launch_layers_depth_grad_as(dim3 grid, size_t lds, hipStream_t st, const TripTable& tt,
                                const LayersDepthGradLaunch& z, const DevDpParams& dp)
{
    if (lds > 48 * 1024)                // deep stacks: opt in to the CU's LDS above the default allowance
        if (int rc = allow_large_lds<&k_render_layers_depth_grad<M, DP, NT>>()) return rc;
    k_render_layers_depth_grad<M, DP, NT><<<grid, kBlock, lds, st>>>(tt, z, dp);
    return 0;
}

template <class M, int DP>
int launch_layers_depth_grad(int nt, dim3 grid, size_t lds, hipStream_t st, const TripTable& tt,
                             const LayersDepthGradLaunch& z, const DevDpParams& dp)
{
    switch (nt) {
    case 1: return launch_layers_depth_grad_as<M, DP, 1>(grid, lds, st, tt, z, dp);
    case 2: return launch_layers_depth_grad_as<M, DP, 2>(grid, lds, st, tt, z, dp);
    case 3: return launch_layers_depth_grad_as<M, DP, 3>(grid, lds, st, tt, z, dp);
    default: return launch_layers_depth_grad_as<M, DP, kMaxPlanes>(grid, lds, st, tt, z, dp);
    }
}

}  // namespace

extern "C" int sdirt_render_plane(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, const float* x1,
                                  const float* y1, double z_sensor, const float* x2, const float* y2, double z_pupil,
                                  int32_t spp, int32_t height, int32_t width, const sdirt_dp_params* dp, double depth,
                                  double inv_texel, const float* tex, int32_t n_tex, int32_t tex_h, int32_t tex_w,
                                  double* num, double* den, float* landing, uint32_t* mask, void* stream)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    if (any_null(x1, y1, x2, y2, tex, num, den)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!all_positive(spp, height, width, n_tex, tex_h, tex_w))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "spp, the sensor's and the texture's extents must be at least 1");
    if ((int64_t)tex_h * tex_w > INT32_MAX) return fail(SDIRT_ERR_INVALID_ARGUMENT, "texture plane above 2^31 texels");
    const int64_t HW = (int64_t)height * width;
    if (HW > (int64_t)INT32_MAX * kBlock) return fail(SDIRT_ERR_INVALID_ARGUMENT, "sensor too large");
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    const DevDpParams dpp = make_dp(dp);
    PlaneLaunch a;
    a.lens = lens->dev; a.K = lens->n_surfaces;
    a.x1 = x1; a.y1 = y1; a.x2 = x2; a.y2 = y2;
    a.z_sensor = (float)z_sensor; a.z_pupil = (float)z_pupil; a.depth = (float)depth; a.inv_texel = (float)inv_texel;
    a.S = spp; a.H = height; a.W = width;
    a.Ht = tex_h; a.Wt = tex_w;
    a.view_stride = (int64_t)n_tex * HW;
    a.den = den; a.landing = landing; a.conv_mask = mask;
    const dim3 grid((unsigned)((HW + kBlock - 1) / kBlock));
    hipStream_t st = as_stream(stream);
    // a launch sums up to kMaxPlanes planes; more planes: further launches over the same rays (den, landing and the
    // masks come out the same from each)
    for (int t0 = 0; t0 < n_tex; t0 += kMaxPlanes) {
        const int nt = n_tex - t0 < kMaxPlanes ? n_tex - t0 : kMaxPlanes;
        a.tex = tex + (int64_t)t0 * tex_h * tex_w;
        a.num = num + (int64_t)t0 * HW;
        with_math(routed_flags(flags, lens), [&](auto m) {
            using Mm = decltype(m);
            if (!dp) return launch_planes<Mm, kDpNone>(nt, grid, st, tt, a, dpp);
            return dpp.big ? launch_planes<Mm, kDpBig>(nt, grid, st, tt, a, dpp)
                           : launch_planes<Mm, kDpSmall>(nt, grid, st, tt, a, dpp);
        });
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}

extern "C" int sdirt_render_layers(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, const float* x1,
                                   const float* y1, double z_sensor, const float* x2, const float* y2, double z_pupil,
                                   int32_t spp, int32_t height, int32_t width, const sdirt_dp_params* dp,
                                   int32_t n_layers, const double* depth, const double* inv_texel, const float* alpha,
                                   const float* tex, int64_t tex_layer_stride, int32_t n_tex, int32_t tex_h,
                                   int32_t tex_w, double* num, double* den, double* cov, float* landing, uint32_t* mask,
                                   void* stream)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    if (any_null(x1, y1, x2, y2, depth, inv_texel, alpha, tex, num, den, cov))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!all_positive(spp, height, width, n_tex, tex_h, tex_w))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "spp, the sensor's and the texture's extents must be at least 1");
    if (n_layers < 1 || n_layers > SDIRT_MAX_LAYERS)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_layers must be in 1 .. SDIRT_MAX_LAYERS");
    if ((int64_t)tex_h * tex_w > INT32_MAX) return fail(SDIRT_ERR_INVALID_ARGUMENT, "texture plane above 2^31 texels");
    if (tex_layer_stride < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "negative tex_layer_stride");
    const int64_t HW = (int64_t)height * width;
    if (HW > (int64_t)INT32_MAX * kBlock) return fail(SDIRT_ERR_INVALID_ARGUMENT, "sensor too large");
    LayersLaunch a;
    for (int l = 0; l < SDIRT_MAX_LAYERS; ++l) {
        const bool used = l < n_layers;
        // the fp32 values the kernel carries the rays to must themselves be negative and strictly descending
        a.depth[l] = used ? (float)depth[l] : 0.0f;
        a.inv_texel[l] = used ? (float)inv_texel[l] : 0.0f;
        if (used && !(a.depth[l] < (l ? a.depth[l - 1] : 0.0f)))
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "layer depths must be negative and strictly descending (nearest first)");
    }
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    const DevDpParams dpp = make_dp(dp);
    a.lens = lens->dev; a.K = lens->n_surfaces;
    a.x1 = x1; a.y1 = y1; a.x2 = x2; a.y2 = y2;
    a.z_sensor = (float)z_sensor; a.z_pupil = (float)z_pupil;
    a.S = spp; a.H = height; a.W = width; a.L = n_layers;
    a.alpha = alpha; a.layer_stride = tex_layer_stride;
    a.Ht = tex_h; a.Wt = tex_w;
    a.view_stride = (int64_t)n_tex * HW;
    a.den = den; a.cov = cov; a.landing = landing; a.conv_mask = mask;
    const dim3 grid((unsigned)((HW + kBlock - 1) / kBlock));
    hipStream_t st = as_stream(stream);
    // more than kMaxPlanes colour planes: further launches over the same rays (den, cov, landing and the masks come out
    // the same from each)
    for (int t0 = 0; t0 < n_tex; t0 += kMaxPlanes) {
        const int nt = n_tex - t0 < kMaxPlanes ? n_tex - t0 : kMaxPlanes;
        a.tex = tex + (int64_t)t0 * tex_h * tex_w;
        a.num = num + (int64_t)t0 * HW;
        with_math(routed_flags(flags, lens), [&](auto m) {
            using Mm = decltype(m);
            if (!dp) return launch_layers<Mm, kDpNone>(nt, grid, st, tt, a, dpp);
            return dpp.big ? launch_layers<Mm, kDpBig>(nt, grid, st, tt, a, dpp)
                           : launch_layers<Mm, kDpSmall>(nt, grid, st, tt, a, dpp);
        });
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}

extern "C" int sdirt_render_layers_grad(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, const float* x1,
                                        const float* y1, double z_sensor, const float* x2, const float* y2,
                                        double z_pupil, int32_t spp, int32_t height, int32_t width,
                                        const sdirt_dp_params* dp, int32_t n_layers, const double* depth,
                                        const double* inv_texel, const float* alpha, const float* tex,
                                        int64_t tex_layer_stride, int32_t n_tex, int32_t tex_h, int32_t tex_w,
                                        const double* gnum, double* galpha, double* gtex, int64_t gtex_layer_stride,
                                        void* stream)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    if (any_null(x1, y1, x2, y2, depth, inv_texel, tex, gnum)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!galpha && !gtex) return fail(SDIRT_ERR_INVALID_ARGUMENT, "galpha and gtex are both null: no gradient is asked for");
    if (!alpha && galpha) return fail(SDIRT_ERR_INVALID_ARGUMENT, "galpha without alpha: an opaque stack has no coverage gradient");
    if (!all_positive(spp, height, width, n_tex, tex_h, tex_w))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "spp, the sensor's and the texture's extents must be at least 1");
    if (n_layers < 1 || n_layers > SDIRT_MAX_LAYERS)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_layers must be in 1 .. SDIRT_MAX_LAYERS");
    if ((int64_t)tex_h * tex_w > INT32_MAX) return fail(SDIRT_ERR_INVALID_ARGUMENT, "texture plane above 2^31 texels");
    if (tex_layer_stride < 0 || gtex_layer_stride < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "negative layer stride");
    const int64_t HW = (int64_t)height * width;
    if (HW > (int64_t)INT32_MAX * kBlock) return fail(SDIRT_ERR_INVALID_ARGUMENT, "sensor too large");
    LayersGradLaunch b;
    for (int l = 0; l < SDIRT_MAX_LAYERS; ++l) {
        const bool used = l < n_layers;
        b.depth[l] = used ? (float)depth[l] : 0.0f;
        b.inv_texel[l] = used ? (float)inv_texel[l] : 0.0f;
        if (used && !(b.depth[l] < (l ? b.depth[l - 1] : 0.0f)))
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "layer depths must be negative and strictly descending (nearest first)");
    }
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    const DevDpParams dpp = make_dp(dp);
    b.lens = lens->dev; b.K = lens->n_surfaces;
    b.x1 = x1; b.y1 = y1; b.x2 = x2; b.y2 = y2;
    b.z_sensor = (float)z_sensor; b.z_pupil = (float)z_pupil;
    b.S = spp; b.H = height; b.W = width; b.L = n_layers;
    b.alpha = alpha; b.layer_stride = tex_layer_stride;
    b.Ht = tex_h; b.Wt = tex_w;
    b.view_stride = (int64_t)n_tex * HW;
    b.galpha = galpha; b.gtex_layer_stride = gtex_layer_stride;
    const dim3 grid((unsigned)((HW + kBlock - 1) / kBlock));
    // the stash of the two walks: two doubles per layer and lane, at most 64 KB; none without a coverage gradient
    const size_t lds = galpha ? (size_t)n_layers * 2 * kBlock * sizeof(double) : 0;
    hipStream_t st = as_stream(stream);
    // more than kMaxPlanes colour planes: further launches over the same rays; the coverage gradient is linear in the
    // planes' D_m, so each launch adds that of its own planes
    for (int t0 = 0; t0 < n_tex; t0 += kMaxPlanes) {
        const int nt = n_tex - t0 < kMaxPlanes ? n_tex - t0 : kMaxPlanes;
        b.tex = tex + (int64_t)t0 * tex_h * tex_w;
        b.gnum = gnum + (int64_t)t0 * HW;
        b.gtex = gtex ? gtex + (int64_t)t0 * tex_h * tex_w : nullptr;
        with_math(routed_flags(flags, lens), [&](auto m) {
            using Mm = decltype(m);
            if (!dp) return launch_layers_grad<Mm, kDpNone>(nt, grid, lds, st, tt, b, dpp);
            return dpp.big ? launch_layers_grad<Mm, kDpBig>(nt, grid, lds, st, tt, b, dpp)
                           : launch_layers_grad<Mm, kDpSmall>(nt, grid, lds, st, tt, b, dpp);
        });
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}

extern "C" int sdirt_render_layers_dp_grad(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, const float* x1,
                                           const float* y1, double z_sensor, const float* x2, const float* y2,
                                           double z_pupil, int32_t spp, int32_t height, int32_t width,
                                           const sdirt_dp_params* dp, int32_t n_layers, const double* depth,
                                           const double* inv_texel, const float* alpha, const float* tex,
                                           int64_t tex_layer_stride, int32_t n_tex, int32_t tex_h, int32_t tex_w,
                                           const double* gnum, const double* gden, double* partial, float* x_tan,
                                           void* stream)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    if (any_null(x1, y1, x2, y2, depth, inv_texel, tex, gnum, partial)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!dp) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null dp: one view with unit weights has no sub-pixel model");
    if (!(dp->r > 0.0)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->r must be > 0");
    if (!(dp->f != dp->h)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "dp->f must differ from dp->h");
    if (!all_positive(spp, height, width, n_tex, tex_h, tex_w))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "spp, the sensor's and the texture's extents must be at least 1");
    if (n_layers < 1 || n_layers > SDIRT_MAX_LAYERS)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_layers must be in 1 .. SDIRT_MAX_LAYERS");
    if ((int64_t)tex_h * tex_w > INT32_MAX) return fail(SDIRT_ERR_INVALID_ARGUMENT, "texture plane above 2^31 texels");
    if (tex_layer_stride < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "negative layer stride");
    const int64_t HW = (int64_t)height * width;
    if (HW > (int64_t)INT32_MAX * kBlock) return fail(SDIRT_ERR_INVALID_ARGUMENT, "sensor too large");
    LayersDpGradLaunch e;
    for (int l = 0; l < SDIRT_MAX_LAYERS; ++l) {
        const bool used = l < n_layers;
        e.depth[l] = used ? (float)depth[l] : 0.0f;
        e.inv_texel[l] = used ? (float)inv_texel[l] : 0.0f;
        if (used && !(e.depth[l] < (l ? e.depth[l - 1] : 0.0f)))
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "layer depths must be negative and strictly descending (nearest first)");
    }
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    const DevDpParams dpp = make_dp(dp);
    const DpGrad q = make_dp_grad(dp);
    e.lens = lens->dev; e.K = lens->n_surfaces;
    e.x1 = x1; e.y1 = y1; e.x2 = x2; e.y2 = y2;
    e.z_sensor = (float)z_sensor; e.z_pupil = (float)z_pupil;
    e.S = spp; e.H = height; e.W = width; e.L = n_layers;
    e.alpha = alpha; e.layer_stride = tex_layer_stride;
    e.Ht = tex_h; e.Wt = tex_w;
    e.view_stride = (int64_t)n_tex * HW;
    e.x_tan = x_tan;
    const int64_t rows = (HW + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)rows);
    hipStream_t st = as_stream(stream);
    // more than kMaxPlanes colour planes: further launches over the same rays, each into a slice of `partial` of its
    // own; the adjoint of den belongs to the ray, not to a plane, and is counted in the first launch only
    for (int t0 = 0; t0 < n_tex; t0 += kMaxPlanes) {
        const int nt = n_tex - t0 < kMaxPlanes ? n_tex - t0 : kMaxPlanes;
        e.tex = tex + (int64_t)t0 * tex_h * tex_w;
        e.gnum = gnum + (int64_t)t0 * HW;
        e.gden = t0 == 0 ? gden : nullptr;
        e.partial = partial + (int64_t)(t0 / kMaxPlanes) * rows * 3;
        with_math(routed_flags(flags, lens), [&](auto m) {
            using Mm = decltype(m);
            return dpp.big ? launch_layers_dp_grad<Mm, kDpBig>(nt, grid, st, tt, e, dpp, q)
                           : launch_layers_dp_grad<Mm, kDpSmall>(nt, grid, st, tt, e, dpp, q);
        });
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}

extern "C" int sdirt_render_layers_depth_grad(const sdirt_lens* lens, const int32_t* trips, uint32_t flags,
                                              const float* x1, const float* y1, double z_sensor, const float* x2,
                                              const float* y2, double z_pupil, int32_t spp, int32_t height,
                                              int32_t width, const sdirt_dp_params* dp, int32_t n_layers,
                                              const double* depth, const double* inv_texel, const float* alpha,
                                              const float* tex, int64_t tex_layer_stride, int32_t n_tex, int32_t tex_h,
                                              int32_t tex_w, const double* gnum, double* partial, float* ray_dir,
                                              void* stream)
{
    if (!lens) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null lens");
    if (any_null(x1, y1, x2, y2, depth, inv_texel, tex, gnum, partial)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (!all_positive(spp, height, width, n_tex, tex_h, tex_w))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "spp, the sensor's and the texture's extents must be at least 1");
    if (n_layers < 1 || n_layers > SDIRT_MAX_LAYERS)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_layers must be in 1 .. SDIRT_MAX_LAYERS");
    if ((int64_t)tex_h * tex_w > INT32_MAX) return fail(SDIRT_ERR_INVALID_ARGUMENT, "texture plane above 2^31 texels");
    if (tex_layer_stride < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "negative layer stride");
    const int64_t HW = (int64_t)height * width;
    if (HW > (int64_t)INT32_MAX * kBlock) return fail(SDIRT_ERR_INVALID_ARGUMENT, "sensor too large");
    LayersDepthGradLaunch z;
    for (int l = 0; l < SDIRT_MAX_LAYERS; ++l) {
        const bool used = l < n_layers;
        z.depth[l] = used ? (float)depth[l] : 0.0f;
        z.inv_texel[l] = used ? (float)inv_texel[l] : 0.0f;
        if (used && !(z.depth[l] < (l ? z.depth[l - 1] : 0.0f)))
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "layer depths must be negative and strictly descending (nearest first)");
    }
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    const DevDpParams dpp = make_dp(dp);
    z.lens = lens->dev; z.K = lens->n_surfaces;
    z.x1 = x1; z.y1 = y1; z.x2 = x2; z.y2 = y2;
    z.z_sensor = (float)z_sensor; z.z_pupil = (float)z_pupil;
    z.S = spp; z.H = height; z.W = width; z.L = n_layers;
    z.alpha = alpha; z.layer_stride = tex_layer_stride;
    z.Ht = tex_h; z.Wt = tex_w;
    z.view_stride = (int64_t)n_tex * HW;
    z.ray_dir = ray_dir;
    const int64_t rows = (HW + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)rows);
    // the lane's 2 L sums, and with a coverage its 2 L stash entries: 4 or 8 KB per layer, at most 128 KB
    const size_t lds = (size_t)n_layers * (alpha ? 4 : 2) * kBlock * sizeof(double);
    hipStream_t st = as_stream(stream);
    // more than kMaxPlanes colour planes: further launches over the same rays, each into a slice of `partial` of its
    // own; every term is linear in q, so the slices add
    for (int t0 = 0; t0 < n_tex; t0 += kMaxPlanes) {
        const int nt = n_tex - t0 < kMaxPlanes ? n_tex - t0 : kMaxPlanes;
        z.tex = tex + (int64_t)t0 * tex_h * tex_w;
        z.gnum = gnum + (int64_t)t0 * HW;
        z.partial = partial + (int64_t)(t0 / kMaxPlanes) * rows * 2 * n_layers;
        const int rc = with_math(routed_flags(flags, lens), [&](auto m) {
            using Mm = decltype(m);
            if (!dp) return launch_layers_depth_grad<Mm, kDpNone>(nt, grid, lds, st, tt, z, dpp);
            return dpp.big ? launch_layers_depth_grad<Mm, kDpBig>(nt, grid, lds, st, tt, z, dpp)
                           : launch_layers_depth_grad<Mm, kDpSmall>(nt, grid, lds, st, tt, z, dpp);
        });
        if (rc) return rc;
        LAUNCH_CHECK();
    }
    return SDIRT_OK;
}
