// What the image-side translation units share (sdirt_render.hip, sdirt_render_grad.hip, sdirt_render_volume.hip):
// the shuffle butterfly, the channel dispatch, the shape rules.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

#include "../../include/sdirt_dp.h"
#include "sdirt_host.hpp"

// The sum over the 64 lanes of a wave, in every lane: a butterfly of wave shuffles, offsets 32 ... 1.  (Not the DPP
// wave_sum of sdirt_render.hip: that one adds in another order.)  The pair form takes both sums level by level.
// k_local_psf_render (sdirt_render.hip) keeps the same loop written out: through this function the compiler lays that
// kernel out differently (same arithmetic), and its ISA is held fixed.
__device__ __forceinline__ float shuffle_sum(float a)
{
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    return a;
}
__device__ __forceinline__ void shuffle_sum(float& a, float& r)
{
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        r += __shfl_xor(r, off);
    }
}

// The run-time channel count to a template argument, as with_math / with_bool (sdirt_host.hpp):
// f(std::integral_constant<int, 1 | 3 | 4>{}).
template <class F>
inline int with_channels(int C, F&& f)
{
    switch (C) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    }
    return fail(SDIRT_ERR_UNSUPPORTED, "channels=%d (supported: 1, 3, 4)", C);
}

// The shape rules of every entry that takes an image [B,C,H,W] and kernels of ks x ks taps: no null pointer, B >= 0,
// H, W >= 1, ks odd.  ks_max > 0 adds the limits of the entries whose launch geometry has them: ks <= ks_max, and B
// and H fit a grid dimension.  channels_here: C is one of with_channels' -- false where the entry finds that out
// later, at its dispatch (an empty batch returns before it).
inline int check_image_call(std::initializer_list<const void*> pointers, int B, int C, int H, int W, int ks, int ks_max,
                            bool channels_here)
{
    for (const void* p : pointers)
        if (!p) return fail(SDIRT_ERR_INVALID_ARGUMENT, "null pointer");
    if (B < 0 || H < 1 || W < 1 || ks < 1 || (ks & 1) == 0)
        return fail(SDIRT_ERR_INVALID_ARGUMENT, "bad shape (ks must be odd, every extent >= 1)");
    if (channels_here)
        if (int rc = with_channels(C, [](auto) { return SDIRT_OK; })) return rc;
    if (ks_max > 0 && ks > ks_max)
        return fail(SDIRT_ERR_UNSUPPORTED, "ks=%d: this entry supports ks <= %d", ks, ks_max);
    if (ks_max > 0 && (B > 65535 || H > 65535))
        return fail(SDIRT_ERR_UNSUPPORTED, "batch=%d height=%d (supported: <= 65535)", B, H);
    return SDIRT_OK;
}
