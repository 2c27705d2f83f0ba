// sdirt_trace_grad.hip -- the backward pass of the staged forward trace (deeplens/optics.py:638-664 with
// surfaces.py:391-679 under autograd): the gradients of a loss with respect to the lens prescription -- every surface's
// d, c, k and ai -- given its gradients with respect to the sensor-plane rays (sdirt_forward_integral_grad_rays).
//
// Three kernels: the recording trace and two backward kernels, k_trace_grad<MP, ETA> and k_trace_grad_points<MP>, which
// walk the record with the same head and the same surface step (load_ray_grad, sensor_adjoint, surface_adjoint: DESIGN.md 7l).
//  k_trace_record: sdirt_trace2sensor's trace (the same device functions, surface by surface, the constants loaded
//      and waited for on the spot) that also stores every ray's (o, d) on ENTRY to each surface and before the final
//      propagation: the checkpoints, [K + 1][6][M] fp32.
//  k_trace_grad: one thread per ray walks the surfaces from last to first.  Per surface it re-runs the no-grad Newton
//      loop from the checkpoint in the forward's own fp32 arithmetic (the trip table decides t1, as in the forward),
//      takes the `_valid` mask and the step clamp of the regain step from those fp32 values, and then differentiates
//        t = t0 + t1 - clamp(ft / (dfdt + 1e-9), +-5),  o' = o + t d,  n = -normalize(N(o'; d, c, k, ai)),
//        d' = sr n + eta (d - cosi n)
//      in float64, carrying the adjoint of (o, d) in registers.  A ray that is dead at the sensor
//      (ra = 0) or lies outside the splat window has no upstream gradient and is skipped; a live ray was valid at every
//      surface, so no validity branch is differentiated.
//  Reduction: the terms of the surface being walked are summed across the wave with shuffles and added, by lane 0, to
//      the wave's own float64 row in LDS; after the walk the rows of the workgroup's waves are added in a fixed order
//      and ONE [K, 3 + SDIRT_MAX_AI] float64 block is stored per workgroup.  No atomics: the same bits every run.
//  k_trace_grad<.., ETA = true>: the same kernel with one more column per surface, dLoss/d eta of its refraction
//      (eta = n1 / n2 as a leaf: deeplens/surfaces.py:44-53, 401-405, 633-669; Python's chain rule takes it to n and V of
//      every medium, basics.py:316-362).
//  k_trace_grad_points: the same walk without parameter columns, one workgroup per (point, spp slice); the adjoint of
//      the ray that enters surface 0 goes on through d = normalize(q - p) to the object point (optics.py:460-494;
//      DESIGN.md 7k).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/sdirt_dp.h"
#include "sdirt_trace.hpp"

using namespace sdirt;

namespace {

constexpr int kParams = 3 + SDIRT_MAX_AI;     // d, c, k, ai2, ai4, ...
constexpr int kAdjWaves = kBlock / 64;

// checkpoint j (entry to surface j; j = K: before the final propagation) of ray i, component c of (o, d)
__device__ __forceinline__ int64_t ckpt_at(int64_t M, int j, int c, int64_t i) { return ((int64_t)j * 6 + c) * M + i; }

__device__ __forceinline__ void store_ckpt(float* __restrict__ ws, int64_t M, int j, int64_t i, const Ray& r)
{
    ws[ckpt_at(M, j, 0, i)] = r.ox; ws[ckpt_at(M, j, 1, i)] = r.oy; ws[ckpt_at(M, j, 2, i)] = r.oz;
    ws[ckpt_at(M, j, 3, i)] = r.dx; ws[ckpt_at(M, j, 4, i)] = r.dy; ws[ckpt_at(M, j, 5, i)] = r.dz;
}

template <class MP>
__global__ void __launch_bounds__(kBlock)
k_trace_record(TripTable trips /* kernarg offset 0 */, const DevSurface* __restrict__ lens, int K, sdirt_rays R,
               sdirt_rays W, int64_t M, uint32_t* __restrict__ conv_mask, float z_sensor, float* __restrict__ ws)
{
    __shared__ uint32_t lds_mask[SDIRT_MAX_SURFACES];
    if (threadIdx.x < SDIRT_MAX_SURFACES) lds_mask[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        Ray r = load_ray(R, i);
        for (int k = 0; k < K; ++k) {
            store_ckpt(ws, M, k, i, r);
            SurfRaw raw;
            surf_issue<true>(raw, lens + k, kernarg_at(0), k);
            surf_wait(raw);
            Surf s;
            s.a = raw.a; s.b = raw.b;
            const uint32_t m = surface_reaction<true, MP>(s, lens + k, surf_trips(raw, k), r, [](uint32_t) {});
            if (conv_mask && m != 0u) lds_or_first_lane(&lds_mask[k], m);
        }
        store_ckpt(ws, M, K, i, r);
        propagate_to<MP>(r, z_sensor);
        store_ray(W, i, r);
    }
    __syncthreads();
    if (conv_mask && (int)threadIdx.x < K && lds_mask[threadIdx.x]) atomicOr(&conv_mask[threadIdx.x], lds_mask[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------
// fp32: the forward's decisions
// ---------------------------------------------------------------------------------------------------------------
struct PolyF {      // the polynomial block through plain (scalar) loads
    float a[kMaxAi], ka[kMaxAi];
    __device__ __forceinline__ float ai(int i) const { return a[i]; }
    __device__ __forceinline__ float kai(int i) const { return ka[i]; }
};

struct Regain {
    float t;        // t0 + t1: where the regain step is evaluated
    bool m;         // the _valid mask of the regain step (surfaces.py:571)
    bool gate;      // the clamp of the step passes the gradient
};

// newton_k's trips and regain step (sdirt_device.hpp) for a LIVE ray under a fixed trip count: the same operations in the
// same order, without the loop bookkeeping (the periodic exit there is exact: it changes no t).
template <class M, bool KGT, class P>
__device__ __forceinline__ Regain newton_regain(const SurfHot& h, const P& pol, const Ray& r, int trips)
{
    const float eps = (float)1e-9;
    const ConicS k{h.c, h.c2, h.onepk, h.d};
    const int deg = (int)((h.flags >> 8) & 15u);
    const float t0 = M::div(k.d - r.oz, r.dz);
    const float dd = r.dx * r.dx + r.dy * r.dy;
    const float dox = r.dx * r.ox + r.dy * r.oy;
    const float bound = KGT ? h.lim_loose : 0.0f;
    float t = t0;
    for (int j = 0; j < trips; ++j) {
        const float nx = r.ox + r.dx * t, ny = r.oy + r.dy * t, nz = r.oz + r.dz * t;
        const float rr = nx * nx + ny * ny;
        const float r2 = (KGT ? rr < bound : rr > bound) ? rr : 0.0f;
        float g, dgd;
        sag_g_dgd<M, KGT, ConicS, false>(k, pol, deg, r2, g, dgd);
        const float ft = (g + k.d) - nz;
        const float dfdt = M::dfdt(dgd, dd * t + dox, r.dz);
        t = t - M::newton_step(ft, dfdt + eps);
    }
    const float t1 = t - t0;
    t = t0 + t1;
    const float nx = r.ox + r.dx * t, ny = r.oy + r.dy * t, nz = r.oz + r.dz * t;
    const float rr = nx * nx + ny * ny;
    Regain out;
    out.t = t;
    out.m = rr < h.lim_tight;
    const float r2 = out.m ? rr : 0.0f;
    float g, dgd;
    sag_g_dgd<M, KGT, ConicS, false>(k, pol, deg, r2, g, dgd);
    const float ft = (g + k.d) - nz;
    const float dfdt = M::dfdt(dgd, dd * t + dox, r.dz);
    const float q = M::div(ft, dfdt + eps);
    out.gate = q >= -kNewtonStepBound && q <= kNewtonStepBound;       // torch.clamp's gradient: 1 inside, bounds included
    return out;
}

// ---------------------------------------------------------------------------------------------------------------
// float64: the derivatives
// ---------------------------------------------------------------------------------------------------------------
// The sag g(r2) = c r2 / (1 + sf) + sum ai r2^(i+1), sf = sqrt(1 - (1 + k) c^2 r2), its r2-derivative gp (what the
// reference's _dgd evaluates: (1 + sf + a/(2 sf)) c / (1 + sf)^2 is c / (2 sf) identically), gp's r2-derivative and
// the derivatives of g and gp in c and k.  pw[j] = r2^j.
struct SagD {
    double g, gp, gpp, g_c, g_k, gp_c, gp_k;
    double pw[kMaxAi + 1];
};

__device__ __forceinline__ SagD sag_d(double c, double kk, const double* a, int deg, double r2)
{
    SagD s;
    const double c3 = c * c * c;
    const double sf = sqrt(1.0 - (1.0 + kk) * r2 * c * c), ops = 1.0 + sf, sf3 = sf * sf * sf;
    s.g = r2 * c / ops;
    s.gp = c / (2.0 * sf);
    s.gpp = (1.0 + kk) * c3 / (4.0 * sf3);
    s.g_c = r2 / (sf * ops);
    s.g_k = r2 * r2 * c3 / (2.0 * sf * ops * ops);
    s.gp_c = 1.0 / (2.0 * sf3);
    s.gp_k = r2 * c3 / (4.0 * sf3);
    s.pw[0] = 1.0;
#pragma unroll
    for (int i = 0; i < kMaxAi; ++i) {
        s.pw[i + 1] = s.pw[i] * r2;
        if (i < deg) {
            s.g += a[i] * s.pw[i + 1];
            s.gp += (double)(i + 1) * a[i] * s.pw[i];
            if (i >= 1) s.gpp += (double)((i + 1) * i) * a[i] * s.pw[i - 1];
        }
    }
    return s;
}

struct Adj {
    double ox, oy, oz, dx, dy, dz;
};

// gbar, hbar: the adjoints of g and gp evaluated at s -> the parameter terms; returns the adjoint of r2
__device__ __forceinline__ double sag_adjoint(const SagD& s, int deg, double gbar, double hbar, double* par)
{
    par[1] += gbar * s.g_c + hbar * s.gp_c;
    par[2] += gbar * s.g_k + hbar * s.gp_k;
#pragma unroll
    for (int i = 0; i < kMaxAi; ++i)
        if (i < deg) par[3 + i] += gbar * s.pw[i + 1] + hbar * (double)(i + 1) * s.pw[i];
    return gbar * s.gp + hbar * s.gpp;
}

// Refraction d' = sr n + eta (d - cosi n), sr = sqrt(1 - eta^2 (1 - cosi^2)), for a unit normal n: given the adjoint
// g of d', the adjoint of d (returned in g) and of n (nb).
__device__ __forceinline__ void refract_adjoint(double eta, double vx, double vy, double vz, double nx, double ny, double nz,
                                                double& gx, double& gy, double& gz, double& nbx, double& nby, double& nbz)
{
    const double cosi = vx * nx + vy * ny + vz * nz;
    const double sr = sqrt(1.0 - eta * eta * (1.0 - cosi * cosi));
    const double gn = gx * nx + gy * ny + gz * nz;
    const double cb = -eta * gn + gn * eta * eta * cosi / sr;         // adjoint of cosi
    const double f = sr - eta * cosi;
    nbx = f * gx + cb * vx; nby = f * gy + cb * vy; nbz = f * gz + cb * vz;
    gx = eta * gx + cb * nx; gy = eta * gy + cb * ny; gz = eta * gz + cb * nz;
}

// The same refraction's derivative in eta (surfaces.py:663-669 with eta a leaf): d d'/d eta = (d - cosi n) - eta (1 - cosi^2) / sr n,
// taken with the adjoint g of d' AS IT ARRIVES, i.e. before refract_adjoint overwrites it.
__device__ __forceinline__ double refract_eta_bar(double eta, double vx, double vy, double vz, double nx, double ny, double nz,
                                                  double gx, double gy, double gz)
{
    const double cosi = vx * nx + vy * ny + vz * nz;
    const double sr = sqrt(1.0 - eta * eta * (1.0 - cosi * cosi));
    const double gn = gx * nx + gy * ny + gz * nz;
    return gx * (vx - cosi * nx) + gy * (vy - cosi * ny) + gz * (vz - cosi * nz) - eta * (1.0 - cosi * cosi) / sr * gn;
}

// o' = o + t d with t = (z - o.z) / d.z: the adjoint of (o, d) from the adjoint of o' (in A.o*) and of d (in A.d*);
// returns the adjoint of z
__device__ __forceinline__ double plane_adjoint(double t, double vx, double vy, double vz, Adj& A)
{
    const double tb = A.ox * vx + A.oy * vy + A.oz * vz;
    A.dx += t * A.ox; A.dy += t * A.oy; A.dz += t * A.oz;
    A.oz -= tb / vz;
    A.dz -= tb * t / vz;
    return tb / vz;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ Ray load_ckpt(const float* __restrict__ ws, int64_t M, int j, int64_t i)
{
    Ray r;
    r.ox = ws[ckpt_at(M, j, 0, i)]; r.oy = ws[ckpt_at(M, j, 1, i)]; r.oz = ws[ckpt_at(M, j, 2, i)];
    r.dx = ws[ckpt_at(M, j, 3, i)]; r.dy = ws[ckpt_at(M, j, 4, i)]; r.dz = ws[ckpt_at(M, j, 5, i)];
    r.ra = 1.0f; r.ob = 1.0f;
    return r;
}

// The adjoint of one curved surface for a live ray: r = the ray on entry, P = its position on the surface (the next
// checkpoint's o), A = in: the adjoint of the ray that leaves, out: of the ray that enters; par += the parameter terms.
// ETA: par[kParams] = the term of eta as well, taken from the adjoint of d' before refract_adjoint overwrites it.
template <bool ETA>
__device__ __forceinline__ void curved_adjoint(const SurfHot& h, const double* a, int deg, const Ray& r, const Regain& rg,
                                               double Px, double Py, double Pz, Adj& A, double* par)
{
    const double D = h.d, c = h.c, kk = h.k, eta = h.eta_f;
    const double ox = r.ox, oy = r.oy, oz = r.oz, vx = r.dx, vy = r.dy, vz = r.dz;
    const bool sphere = (h.flags & 3u) == 1u;
    // ---- refraction at P
    double Nx, Ny, Nz;
    SagD sn;
    const double sg = c > 0.0 ? 2.0 : -2.0;
    if (sphere) {
        Nx = sg * Px; Ny = sg * Py; Nz = sg * Pz - sg * (D + 1.0 / c);
    } else {
        sn = sag_d(c, kk, a, deg, Px * Px + Py * Py);
        Nx = 2.0 * sn.gp * Px; Ny = 2.0 * sn.gp * Py; Nz = -1.0;
    }
    const double nrm = sqrt(Nx * Nx + Ny * Ny + Nz * Nz);
    const double nx = -Nx / nrm, ny = -Ny / nrm, nz = -Nz / nrm;       // forward: the normal is negated (surfaces.py:656)
    double nbx, nby, nbz;
    if constexpr (ETA) par[kParams] = refract_eta_bar(eta, vx, vy, vz, nx, ny, nz, A.dx, A.dy, A.dz);
    refract_adjoint(eta, vx, vy, vz, nx, ny, nz, A.dx, A.dy, A.dz, nbx, nby, nbz);
    const double nn = nbx * nx + nby * ny + nbz * nz;
    const double Nbx = -(nbx - nn * nx) / nrm, Nby = -(nby - nn * ny) / nrm, Nbz = -(nbz - nn * nz) / nrm;
    if (sphere) {
        A.ox += sg * Nbx; A.oy += sg * Nby; A.oz += sg * Nbz;
        par[0] -= sg * Nbz;
        par[1] += sg * Nbz / (c * c);
    } else {
        const double hb = 2.0 * (Nbx * Px + Nby * Py);
        const double r2b = sag_adjoint(sn, deg, 0.0, hb, par);
        A.ox += 2.0 * sn.gp * Nbx + 2.0 * Px * r2b;
        A.oy += 2.0 * sn.gp * Nby + 2.0 * Py * r2b;
    }
    // ---- intersection: P = o + t2 d, t2 = t - clamp(ft / (dfdt + eps)), everything at t = t0 + t1
    const double t = rg.t, eps = (double)(float)1e-9;
    const double X = ox + vx * t, Y = oy + vy * t;
    const double mk = rg.m ? 1.0 : 0.0;
    const SagD sa = sag_d(c, kk, a, deg, mk * (X * X + Y * Y));
    const double ft = sa.g + D - (oz + vz * t);
    const double dd = vx * vx + vy * vy;
    const double dr2dt = 2.0 * (dd * t + (vx * ox + vy * oy));
    const double B = sa.gp * dr2dt - vz + eps;
    const double q = ft / B;
    const double t2 = t - (rg.gate ? q : (q > 0.0 ? (double)kNewtonStepBound : -(double)kNewtonStepBound));
    const double t2b = A.ox * vx + A.oy * vy + A.oz * vz;
    A.dx += t2 * A.ox; A.dy += t2 * A.oy; A.dz += t2 * A.oz;
    double tb = t2b;
    const double qb = rg.gate ? -t2b : 0.0;
    const double ftb = qb / B, dfb = -qb * ft / (B * B);
    A.dz -= dfb;
    const double drb = dfb * sa.gp;
    tb += drb * 2.0 * dd;
    A.dx += drb * 2.0 * (2.0 * vx * t + ox); A.dy += drb * 2.0 * (2.0 * vy * t + oy);
    A.ox += drb * 2.0 * vx; A.oy += drb * 2.0 * vy;
    par[0] += ftb;
    const double r2b = sag_adjoint(sa, deg, ftb, dfb * dr2dt, par);
    const double Xb = r2b * 2.0 * X * mk, Yb = r2b * 2.0 * Y * mk, Zb = -ftb;
    A.ox += Xb; A.oy += Yb; A.oz += Zb;
    A.dx += Xb * t; A.dy += Yb * t; A.dz += Zb * t;
    tb += Xb * vx + Yb * vy + Zb * vz;
    // t = t0 + t1, t0 = (D - o.z) / d.z; t1 carries no gradient
    const double t0 = (D - oz) / vz;
    par[0] += tb / vz;
    A.oz -= tb / vz;
    A.dz -= tb * t0 / vz;
}

// ---------------------------------------------------------------------------------------------------------------
// the walk: one head, one surface step, shared by the kernels below
// ---------------------------------------------------------------------------------------------------------------
// The upstream gradient of ray i (o.x, o.y, d.x, d.z of the sensor-plane ray) into A; returns whether the ray has one.
// `in_range`: the lane has a ray at all.
__device__ __forceinline__ bool load_ray_grad(bool in_range, const float* __restrict__ ra, const float* __restrict__ ray_grad,
                                              int64_t M, int64_t i, Adj& A)
{
    if (!(in_range && ra[i] != 0.0f)) return false;
    A.ox = ray_grad[i]; A.oy = ray_grad[M + i]; A.dx = ray_grad[2 * M + i]; A.dz = ray_grad[3 * M + i];
    return A.ox != 0.0 || A.oy != 0.0 || A.dx != 0.0 || A.dz != 0.0;
}

// The final propagation to the sensor plane (in the ray only), and P = checkpoint K's o: where the ray left surface K - 1.
__device__ __forceinline__ void sensor_adjoint(const float* __restrict__ ws, int64_t M, int K, int64_t ii, float z_sensor,
                                               Adj& A, float& Px, float& Py, float& Pz)
{
    const Ray r = load_ckpt(ws, M, K, ii);
    const double t = ((double)z_sensor - (double)r.oz) / (double)r.dz;
    (void)plane_adjoint(t, r.dx, r.dy, r.dz, A);
    Px = ws[ckpt_at(M, K, 0, ii)]; Py = ws[ckpt_at(M, K, 1, ii)]; Pz = ws[ckpt_at(M, K, 2, ii)];
}

// One step of the walk, surface k of ray ii: A = in: the adjoint of the ray that leaves the surface, out: of the ray
// that enters it; par[NP] = the surface's parameter terms of this ray (zeroed here; with ETA, par[kParams] = eta's);
// P = in: the ray's position on the surface, out: on the surface before it (checkpoint k's o).
template <class MP, bool ETA, int NP>
__device__ __forceinline__ void surface_adjoint(const TripTable& trips, const DevSurface* __restrict__ lens, int k,
                                                const float* __restrict__ ws, int64_t M, int64_t ii, float& Px, float& Py,
                                                float& Pz, Adj& A, double* par)
{
    const SurfHot& h = lens[k].h;
    const Ray r = load_ckpt(ws, M, k, ii);
    const int kind = (int)(h.flags & 3u), deg = (int)((h.flags >> 8) & 15u);
#pragma unroll
    for (int c = 0; c < NP; ++c) par[c] = 0.0;
    if (kind == 0) {
        if (h.flags & kFlagRefract) {
            double nbx, nby, nbz;
            if constexpr (ETA) par[kParams] = refract_eta_bar((double)h.eta_f, r.dx, r.dy, r.dz, 0.0, 0.0, 1.0, A.dx, A.dy, A.dz);
            refract_adjoint((double)h.eta_f, r.dx, r.dy, r.dz, 0.0, 0.0, 1.0, A.dx, A.dy, A.dz, nbx, nby, nbz);
        }
        const double t = ((double)h.d - (double)r.oz) / (double)r.dz;
        par[0] = plane_adjoint(t, r.dx, r.dy, r.dz, A);
    } else {
        const int trip = (int)(int8_t)(trips.w[k >> 2] >> ((k & 3) * 8));
        double a[kMaxAi];
        Regain rg;
        if (deg > 0) {
            PolyF pol;
#pragma unroll
            for (int c = 0; c < kMaxAi; ++c) { pol.a[c] = lens[k].p.ai[c]; pol.ka[c] = lens[k].p.kai[c]; a[c] = pol.a[c]; }
            rg = (h.flags & kFlagKgtM1) ? newton_regain<MP, true>(h, pol, r, trip) : newton_regain<MP, false>(h, pol, r, trip);
        } else {
#pragma unroll
            for (int c = 0; c < kMaxAi; ++c) a[c] = 0.0;
            rg = (h.flags & kFlagKgtM1) ? newton_regain<MP, true>(h, NoPoly{}, r, trip)
                                        : newton_regain<MP, false>(h, NoPoly{}, r, trip);
        }
        curved_adjoint<ETA>(h, a, deg, r, rg, Px, Py, Pz, A, par);
    }
    Px = r.ox; Py = r.oy; Pz = r.oz;
}

// The surface parameters' kernel.  ETA: one more column per surface, dLoss/d eta of its refraction, for every surface
// that refracts (every curved one, and a plane between different media; the stop's stays exactly 0).
template <class MP, bool ETA>
__global__ void __launch_bounds__(kBlock)
k_trace_grad(TripTable trips, const DevSurface* __restrict__ lens, int K, const float* __restrict__ ws,
             const float* __restrict__ ra, const float* __restrict__ ray_grad, int64_t M, float z_sensor,
             double* __restrict__ partial)
{
    constexpr int NP = kParams + (ETA ? 1 : 0);
    __shared__ double acc[kAdjWaves][SDIRT_MAX_SURFACES][NP];
    for (int e = threadIdx.x; e < kAdjWaves * SDIRT_MAX_SURFACES * NP; e += kBlock) (&acc[0][0][0])[e] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < M; base += (int64_t)gridDim.x * kBlock) {
        const int64_t i = base + threadIdx.x;
        Adj A{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const bool live = load_ray_grad(i < M, ra, ray_grad, M, i, A);
        if (__ballot(live) == 0ull) continue;
        const int64_t ii = i < M ? i : M - 1;                 // idle lanes read a ray that exists and contribute nothing
        float Px, Py, Pz;
        sensor_adjoint(ws, M, K, ii, z_sensor, A, Px, Py, Pz);
        for (int k = K - 1; k >= 0; --k) {
            const SurfHot& h = lens[k].h;       // (read before the step, which decodes the same two: one decode)
            const int kind = (int)(h.flags & 3u), deg = (int)((h.flags >> 8) & 15u);
            double par[NP];
            surface_adjoint<MP, ETA, NP>(trips, lens, k, ws, M, ii, Px, Py, Pz, A, par);
            // the columns this surface owns (Aspheric.activate_grad, surfaces.py:837-860): d; c unless a plane; k of an
            // asphere with k != 0; its ai; with ETA, eta if it refracts.  Every other column stays exactly 0.
            const bool own_k = kind == 2 && h.k != 0.0f, own_eta = ETA && (h.flags & kFlagRefract) != 0u;
#pragma unroll
            for (int c = 0; c < NP; ++c) {
                const bool own = c == 0 || (c == 1 && kind != 0) || (c == 2 && own_k) || (c >= 3 && c < kParams && c - 3 < deg) ||
                                 (c == kParams && own_eta);
                if (!own) continue;                                          // wave-uniform
                const double v = wave_sum(live ? par[c] : 0.0);
                if (lane == 0) acc[wave][k][c] += v;
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < K * NP; e += kBlock) {
        const int k = e / NP, c = e - k * NP;
        double v = 0.0;
        for (int w = 0; w < kAdjWaves; ++w) v += acc[w][k][c];
        partial[(int64_t)blockIdx.x * K * NP + e] = v;
    }
}

// The walk once more, for the OBJECT POINTS: no parameter columns, no LDS rows.  One workgroup per (point, slice of the
// spp axis) of a point-major bundle (ray (s, n) = n S + s).  After surface 0 the adjoint A is that of the sampled ray
// (o0, d0) = (p, normalize(q_s - p)), q_s = (x2[s], y2[s], pupil_z) (deeplens/optics.py:490-494, basics.py:245), so the
// ray's term of the point's adjoint is A.o - (A.d - d0 (d0 . A.d)) / |q_s - p|, float64 from the fp32 p (checkpoint 0's
// o), x2, y2 and pupil_z.  A thread adds its rays' terms in order, the wave sums by shuffles, the four waves meet in
// LDS: ONE float64 triple per (point, slice), no atomics, nothing pre-zeroed.  A kernel of its own for its grid,
// reduction and tail; the head and the surface step are k_trace_grad's.
template <class MP>
__global__ void __launch_bounds__(kBlock)
k_trace_grad_points(TripTable trips, const DevSurface* __restrict__ lens, int K, const float* __restrict__ ws,
                    const float* __restrict__ ra, const float* __restrict__ ray_grad, int64_t M, int64_t S, int nslices,
                    int64_t chunk, float z_sensor, const float* __restrict__ x2, const float* __restrict__ y2, float pupil_z,
                    double* __restrict__ partial)
{
    __shared__ double red[kAdjWaves][3];
    const int64_t n = blockIdx.x / (uint32_t)nslices;
    const int j = (int)(blockIdx.x - (uint32_t)n * nslices);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[3] = {0.0, 0.0, 0.0};
    const int64_t s_begin = (int64_t)j * chunk, s_end = min(S, s_begin + chunk);
    for (int64_t base = s_begin; base < s_end; base += kBlock) {
        const int64_t s = base + threadIdx.x;
        const int64_t ss = s < s_end ? s : s_end - 1;         // idle lanes read a ray that exists and contribute nothing
        const int64_t ii = n * S + ss;
        Adj A{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const bool live = load_ray_grad(s < s_end, ra, ray_grad, M, ii, A);
        if (__ballot(live) == 0ull) continue;
        float Px, Py, Pz;
        sensor_adjoint(ws, M, K, ii, z_sensor, A, Px, Py, Pz);
        for (int k = K - 1; k >= 0; --k) {
            double par[kParams];                         // (the parameter terms are dead: nothing reads par)
            surface_adjoint<MP, false, kParams>(trips, lens, k, ws, M, ii, Px, Py, Pz, A, par);
        }
        if (live) {
            // (Px, Py, Pz) is checkpoint 0's o: the point itself
            const double vx = (double)x2[ss] - (double)Px, vy = (double)y2[ss] - (double)Py, vz = (double)pupil_z - (double)Pz;
            const double len = sqrt(vx * vx + vy * vy + vz * vz);
            const double ux = vx / len, uy = vy / len, uz = vz / len;
            const double ud = ux * A.dx + uy * A.dy + uz * A.dz;
            acc[0] += A.ox - (A.dx - ux * ud) / len;
            acc[1] += A.oy - (A.dy - uy * ud) / len;
            acc[2] += A.oz - (A.dz - uz * ud) / len;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = wave_sum(acc[c]);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = 0.0;
        for (int w = 0; w < kAdjWaves; ++w) v += red[w][threadIdx.x];
        partial[(n * nslices + j) * 3 + threadIdx.x] = v;
    }
}

int grad_workgroups(int64_t M, int ncu)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((M + kBlock - 1) / kBlock, 8 * (int64_t)ncu));
}

}  // namespace

extern "C" {

int64_t sdirt_trace2sensor_grad_workspace_bytes(int64_t n_rays, int32_t n_surfaces)
{
    if (n_rays < 0 || n_surfaces < 1 || n_surfaces > SDIRT_MAX_SURFACES) return 0;
    return (int64_t)sizeof(float) * 6 * (n_surfaces + 1) * n_rays;
}

int32_t sdirt_trace2sensor_grad_workgroups(int64_t n_rays, int32_t n_cus)
{
    if (n_rays < 0 || n_cus < 1) return 0;
    return grad_workgroups(n_rays, n_cus);
}

int sdirt_trace2sensor_record(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, double d_sensor, sdirt_rays rays,
                              sdirt_rays out, int64_t M, uint32_t* conv_mask, void* workspace, void* stream)
{
    if (!lens || !workspace) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = check_rays(rays)) return rc;
    if (int rc = check_rays(out)) return rc;
    if ((rays.obliq == nullptr) != (out.obliq == nullptr))
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "obliq must be present in both bundles or in neither");
    TripTable tt;
    if (int rc = make_trips(lens, trips, tt)) return rc;
    if (M < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_rays < 0");
    if (M == 0) return SDIRT_OK;
    with_math(routed_flags(flags, lens), [&](auto m) {
        k_trace_record<decltype(m)><<<grid_for(M, kBlock), kBlock, 0, as_stream(stream)>>>(
            tt, lens->dev, lens->n_surfaces, rays, out, M, conv_mask, (float)d_sensor, (float*)workspace);
        return 0;
    });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

// What every backward walk checks first.  `pointers`: all of the entry's pointer arguments are there.
static int walk_arguments(bool pointers, const sdirt_lens* lens, const int32_t* trips, TripTable& tt)
{
    if (!pointers) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = make_trips(lens, trips, tt)) return rc;
    for (int k = 0; k < lens->n_surfaces; ++k)
        if (trips && trips[k] < 0)
            return fail(SDIRT_ERR_UNSUPPORTED, "trips[%d] < 0: the per-wave trip count of the speed mode is not recorded", k);
    return SDIRT_OK;
}

// sdirt_trace2sensor_grad (eta = false) and sdirt_trace2sensor_grad_eta (true): one argument check, one launch
static int launch_trace_grad(bool eta, const sdirt_lens* lens, const int32_t* trips, uint32_t flags, double d_sensor,
                             const void* workspace, const float* ra, const float* ray_grad, int64_t M, double* partial,
                             int32_t n_workgroups, void* stream)
{
    TripTable tt;
    if (int rc = walk_arguments(lens && workspace && ra && ray_grad && partial, lens, trips, tt)) return rc;
    if (M < 0) return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_rays < 0");
    int ncu = 0;
    if (int rc = device_cus(&ncu)) return rc;
    const int grid = grad_workgroups(M, ncu);
    if (n_workgroups != grid)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_workgroups=%d, the launch has %d (sdirt_trace2sensor_grad_workgroups)",
                    n_workgroups, grid);
    with_math(routed_flags(flags, lens), [&](auto m) {
        auto* kernel = eta ? k_trace_grad<decltype(m), true> : k_trace_grad<decltype(m), false>;
        kernel<<<grid, kBlock, 0, as_stream(stream)>>>(
            tt, lens->dev, lens->n_surfaces, (const float*)workspace, ra, ray_grad, M, (float)d_sensor, partial);
        return 0;
    });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

int sdirt_trace2sensor_grad(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, double d_sensor,
                            const void* workspace, const float* ra, const float* ray_grad, int64_t M, double* partial,
                            int32_t n_workgroups, void* stream)
{
    return launch_trace_grad(false, lens, trips, flags, d_sensor, workspace, ra, ray_grad, M, partial, n_workgroups, stream);
}

int sdirt_trace2sensor_grad_eta(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, double d_sensor,
                                const void* workspace, const float* ra, const float* ray_grad, int64_t M, double* partial,
                                int32_t n_workgroups, void* stream)
{
    return launch_trace_grad(true, lens, trips, flags, d_sensor, workspace, ra, ray_grad, M, partial, n_workgroups, stream);
}

int sdirt_trace2sensor_grad_points(const sdirt_lens* lens, const int32_t* trips, uint32_t flags, double d_sensor,
                                   const void* workspace, const float* ra, const float* ray_grad, int64_t S, int64_t N,
                                   const float* x2, const float* y2, double pupil_z, double* partial, int32_t n_slices,
                                   void* stream)
{
    TripTable tt;
    if (int rc = walk_arguments(lens && workspace && ra && ray_grad && x2 && y2 && partial, lens, trips, tt)) return rc;
    if (S < 0 || N < 0 || N > (1ll << 30)) return fail(SDIRT_ERR_INVALID_ARGUMENT, "spp < 0 or n_points out of range");
    if (N == 0) return SDIRT_OK;
    int ncu = 0;
    if (int rc = device_cus(&ncu)) return rc;
    const int32_t ns = sdirt_forward_integral_grad_slices(N, S, ncu);
    if (n_slices != ns)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_slices=%d, the launch has %d (sdirt_forward_integral_grad_slices)", n_slices, ns);
    if (N * (int64_t)ns > 0x7fffffffll) return fail(SDIRT_ERR_INVALID_ARGUMENT, "n_points * n_slices exceeds the grid");
    // the slices cover the spp axis in runs of `chunk` samples (a trailing slice may be empty: it stores zeros)
    const int64_t chunk = std::max<int64_t>(1, (S + ns - 1) / ns);
    with_math(routed_flags(flags, lens), [&](auto m) {
        k_trace_grad_points<decltype(m)><<<(unsigned)(N * ns), kBlock, 0, as_stream(stream)>>>(
            tt, lens->dev, lens->n_surfaces, (const float*)workspace, ra, ray_grad, S * N, S, ns, chunk, (float)d_sensor, x2, y2,
            (float)pupil_z, partial);
        return 0;
    });
    LAUNCH_CHECK();
    return SDIRT_OK;
}

}  // extern "C"
