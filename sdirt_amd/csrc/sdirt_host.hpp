// Host-side helpers shared by the translation units of libsdirt_dp.so: the thread-local
// error text behind sdirt_last_error(), status macros, stream cast.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include <cstdint>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/sdirt_dp.h"
#include "sdirt_device.hpp"

inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(SDIRT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                  \
    } while (0)

#define LAUNCH_CHECK()                                                                  \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess)                                                           \
            return fail(SDIRT_ERR_HIP, "kernel launch failed: %s (%s:%d)",              \
                        hipGetErrorString(e_), __FILE__, __LINE__);                     \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Compute units of the CURRENT device (the binding makes the stream's device current for every call): 256 on an
// MI355X in SPX mode, 32 per XCD of a partitioned one.  Asked once per device, launch geometry is sized from it.
constexpr int kMaxDevices = 64;
inline int device_cus(int* out)
{
    static int cached[kMaxDevices] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev >= 0 && dev < kMaxDevices && cached[dev] > 0) { *out = cached[dev]; return SDIRT_OK; }
    int n = 0;
    HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    if (n < 1) return fail(SDIRT_ERR_HIP, "device %d reports %d compute units", dev, n);
    if (dev >= 0 && dev < kMaxDevices) cached[dev] = n;
    *out = n;
    return SDIRT_OK;
}
// Opt a kernel in to more dynamic LDS than the default 48 KiB allowance (up to the CU's 160 KiB): once per kernel
// instantiation, device and size -- the largest size asked for so far is remembered per device, a later launch that
// needs more sets the attribute again.  (Concurrent host threads: the attribute call is idempotent, the remembered
// size only ever grows.)
template <auto Kernel>
inline int allow_large_lds(int bytes = 160 * 1024 - 1024)
{
    static std::atomic<int> allowed[kMaxDevices] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < kMaxDevices;
    if (known && allowed[dev].load(std::memory_order_acquire) >= bytes) return SDIRT_OK;
    HIP_TRY(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (known) {
        int seen = allowed[dev].load(std::memory_order_relaxed);
        while (seen < bytes && !allowed[dev].compare_exchange_weak(seen, bytes, std::memory_order_release)) {}
    }
    return SDIRT_OK;
}

// for the pure sizing helpers that may be asked before any device exists (sdirt_psf_spp_slices): MI355X's 256
inline int device_cus_or_default()
{
    int n = 0;
    return device_cus(&n) == SDIRT_OK ? n : 256;
}


// The dual-pixel sub-pixel weights (sl, sr) of k_psf_lr as a table over x_tan (sdirt_psf.hip: dp_table_for): a
// property of the SENSOR (h, f, w, r), built once per parameter set and kept with the lens handle the call renders
// through.  The device buffer is allocated with the handle (data-path calls never allocate) and holds
// kDpTableEntries + 1 float2 whatever the parameters, so that no index the kernel can form leaves it.
constexpr int kDpTableEntries = 1 << 18;          // capacity: 2 MiB; a parameter set uses 2 * half + 1 entries of it
struct DpWeightTable {
    float2* dev = nullptr;                        // [kDpTableEntries + 1] (sl, sr) at x_tan = (i - half) / scale
    bool built = false;
    uint64_t key[4] = {};                         // bit patterns of the doubles (h, f, w, r) the entries were built from
    int half = 0;                                 // entries on either side of x_tan = 0
    int log2_scale = 0;                           // cells per unit of x_tan: a power of two, the index is exact in fp32
    hipEvent_t ready = nullptr;                   // recorded behind the build on the stream that ran it
    std::vector<hipStream_t> synced;              // streams already ordered behind `ready`
    std::mutex lock;
};

// A prescription at one wavelength: the device table the kernels read and its host mirror.
struct sdirt_lens {
    int32_t n_surfaces;
    sdirt::DevSurface* dev;               // device table [n_surfaces]
    std::vector<sdirt::DevSurface> host;  // host mirror
    mutable DpWeightTable dp_table;       // filled by the PSF calls that render through this handle
    bool strict_ieee;                     // a surface can reach the seeded sag quotient's exception: every launch runs Ieee
};

// The flags a launch through these handles runs under: SDIRT_PSF_STRICT_IEEE is added for a lens that
// sdirt_lens_create marked (sdirt_trace.hip: sag_seed_exception) -- about one curvature in four million.  Taken once
// at the head of a launcher, so that with_math and everything else that reads the flag (the dual-pixel weight table)
// see the same policy.
inline uint32_t routed_flags(uint32_t flags, const sdirt_lens* lens) { return lens && lens->strict_ieee ? flags | SDIRT_PSF_STRICT_IEEE : flags; }
inline uint32_t routed_flags(uint32_t flags, const sdirt_lens* const* lens, int n)
{
    for (int i = 0; lens && i < n; ++i) flags = routed_flags(flags, lens[i]);
    return flags;
}

// Newton trip counts of one launch, one signed byte per surface, passed by value at a FIXED
// offset of the kernel-argument segment; the kernels read the dword of surface k from there
// with a scalar load that shares the round trip of the surface's constant block (a byte-indexed
// by-value table made the compiler issue a vector load and wait for it once per surface).
struct alignas(64) TripTable {
    uint32_t w[SDIRT_MAX_SURFACES / 4];
};
static_assert(sizeof(TripTable) == 64, "layout");

inline int make_trips(const sdirt_lens* lens, const int32_t* trips, TripTable& tt)
{
    for (int k = 0; k < SDIRT_MAX_SURFACES / 4; ++k) tt.w[k] = 0;
    for (int k = 0; k < lens->n_surfaces; ++k) {
        int v = trips ? trips[k] : SDIRT_NEWTON_MAXITER;
        if (v < -SDIRT_NEWTON_MAXITER || v > SDIRT_NEWTON_MAXITER)
            return fail(SDIRT_ERR_INVALID_ARGUMENT, "trips[%d]=%d outside [-%d,%d]", k, v,
                        SDIRT_NEWTON_MAXITER, SDIRT_NEWTON_MAXITER);
        tt.w[k >> 2] |= (uint32_t)(uint8_t)(int8_t)v << ((k & 3) * 8);
    }
    return SDIRT_OK;
}

constexpr int kBlock = 256;
// Workgroup size of the two fused kernels.  512 threads = 8 waves share one pair of
// L/R tiles (33.8 KB at ks 65): 4 workgroups = 32 waves per CU = 8 per SIMD; both
// kernels need <= 43 VGPRs.  Measured on config 2: k_psf_lr 12.69 ms at 256 threads
// (LDS-limited to 4 waves/SIMD), 11.76 ms at 512, 15.7 ms at 1024.
constexpr int kFused = 512;

inline int grid_for(int64_t work, int block, int cap = 256 * 16)
{
    int64_t g = (work + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

inline int check_rays(const sdirt_rays& R)
{
    if (!R.ox || !R.oy || !R.oz || !R.dx || !R.dy || !R.dz || !R.ra)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "sdirt_rays has a null array");
    return SDIRT_OK;
}

// every component array on a 16-byte boundary (dwordx4 access)
inline bool rays_aligned16(const sdirt_rays& R)
{
    const uintptr_t a = (uintptr_t)R.ox | (uintptr_t)R.oy | (uintptr_t)R.oz | (uintptr_t)R.dx | (uintptr_t)R.dy |
                        (uintptr_t)R.dz | (uintptr_t)R.ra | (uintptr_t)R.obliq;
    return (a & 15) == 0;
}

// The device-side constants of a dual-pixel parameter block (NULL: the reference's defaults) and of a splat window,
// as every kernel that splats or differentiates a splat (sdirt_psf.hip, sdirt_grad.hip) computes them.
inline sdirt::DevDpParams make_dp(const sdirt_dp_params* dp)
{
    sdirt::DevDpParams p;
    const double h = dp ? dp->h : 0.78, f = dp ? dp->f : 1.44, w = dp ? dp->w : 0.3,
                 r = dp ? dp->r : 0.5;
    p.h = (float)h; p.f = (float)f; p.w = (float)w; p.r = (float)r;
    p.fmh = (float)(f - h);
    p.rr = p.r * p.r;
    p.big = r > 0.5;
    p.have_r = dp != nullptr;
    int ex = 0;
    p.r_pow2 = std::frexp(p.r, &ex) == 0.5f;
    p.inv_r = 1.0f / p.r;
    p.tr = std::asin((1.0f / p.r) * 0.5f);
    p.tl = (float)3.141592653589793 - p.tr;
    return p;
}

inline sdirt::SplatGeom make_geom(double ps, int ks)
{
    sdirt::SplatGeom g;
    const double hi = (ks / 2.0 - 0.5) * ps, lo = (-ks / 2.0 + 0.5) * ps;
    g.lim = (float)(hi - 0.01 * ps);
    g.x_min = (float)lo;
    g.y_max = (float)hi;
    g.dx_rng = (float)(hi - lo);
    g.dy_rng = (float)(lo - hi);
    g.ksm1 = (float)(ks - 1);
    g.ks = ks;
    return g;
}

// Run-time switches to template arguments, for the launchers that pick one instantiation of a kernel template:
// f(sdirt::Lean{}) or -- SDIRT_PSF_STRICT_IEEE -- f(sdirt::Ieee{}); f(std::true_type{}) or f(std::false_type{}).
template <class F>
inline int with_math(uint32_t flags, F&& f)
{
    return (flags & SDIRT_PSF_STRICT_IEEE) ? f(sdirt::Ieee{}) : f(sdirt::Lean{});
}
template <class F>
inline int with_bool(bool b, F&& f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}
// ... and f(Elem<T, lanes>{}) for the kernels over fp16 / fp32 tensors that give a thread either one 16-byte group of
// elements (wide) or a single one: _Float16 / 8, _Float16 / 1, float / 4, float / 1.
template <class T, int VL>
struct Elem {
    using type = T;
    static constexpr int lanes = VL;
};
template <class F>
inline int with_elem(bool half, bool wide, F&& f)
{
    if (half) return wide ? f(Elem<_Float16, 8>{}) : f(Elem<_Float16, 1>{});
    return wide ? f(Elem<float, 4>{}) : f(Elem<float, 1>{});
}
// ... and what the launchers around them share: the element type of a with_bool(half precision?) tag, the two kinds of
// argument check (a null pointer among these; every extent at least 1), the status behind a launch.
template <class Half>
using half_or_float = std::conditional_t<Half::value, _Float16, float>;
template <class... P>
inline bool any_null(P... p) { return (... || !p); }
template <class... N>
inline bool all_positive(N... n) { return (... && (n >= 1)); }
inline int launched()
{
    LAUNCH_CHECK();
    return SDIRT_OK;
}
// May `count` fp16 / fp32 elements behind the pointers OR-ed into `ptrs` be walked in 16-byte groups -- a whole number
// of them, at most `max_groups`, every pointer on a 16-byte boundary?
inline bool groups_of_16_bytes(int64_t count, bool half, uintptr_t ptrs, int64_t max_groups = INT64_MAX)
{
    const int vl = half ? 8 : 4;
    return count % vl == 0 && count / vl <= max_groups && (ptrs & 15) == 0;
}

inline int check_ks(int ks, int max_ks = SDIRT_MAX_KS)
{
    if (ks < 2 || ks > max_ks)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "ks=%d outside [2,%d]", ks, max_ks);
    return SDIRT_OK;
}
