// splat_pick_math.h -- the arithmetic of the pick (splat_pick_device, splat_pick.hip): the key the hits of a pixel are ordered
// by, the fragment a hit is judged with, and the coverage chain the surface is found on.  Plain C++, __host__ __device__: the
// same text compiles for the CPU (tests/native/pick_math_probe.hip, tests/test_pick_math_host.py).  Built without
// contraction, like everything that has to match the oracle bit for bit.
#pragma once
#include <stdint.h>

#include "splat_device_math.h"

// ---- the order of a pixel's hits -------------------------------------------------------------------------------------
// Nearest first: the reverse of the order the reference draws in (stable, ascending view-space z), so descending depth and,
// among equal depths, descending original index.  One unsigned 64-bit key says both -- a LARGER key is NEARER: the depth's
// order-preserving integer image above the index.  Float comparison makes -0.0 and +0.0 equal, so the zero's sign is
// dropped before the bits are taken; a NaN has no place in the order and never gets here (it is never visible).  The keys of
// one pixel are distinct because the indices are.
__host__ __device__ __forceinline__ uint32_t pick_depth_key(float depth) {
    uint32_t b = __builtin_bit_cast(uint32_t, depth);
    if (b == 0x80000000u) b = 0u;                              // -0.0 ties with +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the depth a key was made of (a -0.0 comes back as +0.0: no hit has one -- tz = 0 leaves no finite record)
__host__ __device__ __forceinline__ float pick_key_depth(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    return __builtin_bit_cast(float, b);
}
__host__ __device__ __forceinline__ uint64_t pick_key(float depth, uint32_t index) {
    return ((uint64_t)pick_depth_key(depth) << 32) | (uint64_t)index;
}
__host__ __device__ __forceinline__ uint32_t pick_key_index(uint64_t key) { return (uint32_t)key; }
__host__ __device__ __forceinline__ float pick_key_depth64(uint64_t key) { return pick_key_depth((uint32_t)(key >> 32)); }

// ---- the fragment ----------------------------------------------------------------------------------------------------
// The reference's fragment() at sample (sx, sy) of the record with centre (cx, cy), half extents (hx, hy), conic (ca, cb, cc)
// and `opacity`: the alpha it is blended with, 0 where there is no fragment (the sample outside the record's rectangle,
// power > 0, alpha < 1/255).  The operations and their order are fragment_alpha's (splat_device_math.h) and the oracle's
// (orc_render's loop), with the y axis's sign taken here rather than folded into cb, and the exponential is ALWAYS exp_libm
// -- glibc's expf bit for bit -- whatever mode the context renders in: every alpha the pick reports is the oracle's.
__host__ __device__ __forceinline__ float pick_fragment(float sx, float sy, float cx, float cy, float hx, float hy, float ca, float cb,
                                                        float cc, float opacity, bool y_up) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long* const tab = EXP2F_TAB;
#else
    const unsigned long long* const tab = EXP2F_TAB_HOST;
#endif
    const float dx = sx - cx;
    const float dy = y_up ? cy - sy : sy - cy;
    if (!(fabsf(dx) <= hx) || !(fabsf(dy) <= hy)) return 0.0f;
    const float power = -0.5f * (ca * dx * dx + cc * dy * dy) - cb * dx * dy;
    if (power > 0.0f) return 0.0f;
    const float alpha = fminf(0.99f, opacity * exp_libm(power, tab));
    if (alpha < 1.0f / 255.0f) return 0.0f;
    return alpha;
}

// ---- the coverage chain ----------------------------------------------------------------------------------------------
// Walking the hits nearest first: T_0 = 1, T_k = T_{k-1} * (1 - alpha_k) in f32 -- the subtraction rounded, then the product --
// and coverage_k = 1 - T_k.  Float transmittance, NOT the reference's blend: that truncates to 8 bits after every splat.
__host__ __device__ __forceinline__ float pick_transmit(float t, float alpha) {
    const float ia = 1.0f - alpha;
    return t * ia;
}
__host__ __device__ __forceinline__ float pick_coverage(float t) { return 1.0f - t; }
