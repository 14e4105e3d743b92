// splat_device_math.h -- the small functions every exactness claim of the compositor ends in: the two
// exponentials, fragment(), blend(), the block coverage test and K1's certain-reject threshold.
// splat_kernels.hip includes it; so does tests/native/device_math_probe.hip, which runs each function alone on
// chosen inputs (tests/test_gpu_device_math.py, tests/test_device_math_host.py).  What is plain C++ is
// __host__ __device__, so that the same text also compiles for the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// K1: fragments with power < reject_threshold(opacity) have alpha < 1/255 for certain (margin 1e-3 >> f32 error)
__host__ __device__ __forceinline__ float reject_threshold(float opacity) {
    return (opacity > 0.0f) ? (logf(1.0f / (255.0f * opacity)) - 1e-3f)
                            : ((opacity <= 0.0f) ? 3.0e38f : -3.0e38f);
}

// Does ANY sample s = lo + k (k = 0..count-1, all exactly representable) satisfy |s - c| <= h ?
// |s - c| grows monotonically (also after f32 rounding) away from c, so testing the one or two
// samples nearest to c is exact.
__host__ __device__ __forceinline__ bool any_sample_covered(float c, float h, float lo, float hi, float off) {
    float s1 = fminf(fmaxf(floorf(c - off) + off, lo), hi);
    float s2 = fminf(s1 + 1.0f, hi);
    return (int)(fabsf(s1 - c) <= h) | (int)(fabsf(s2 - c) <= h);
}

// exp(x) for the compositor: the same reduction ocml's expf performs (2^(x*log2e) with a
// compensated product, v_exp_f32 on the fractional part, ldexp) without its overflow/underflow
// selects -- x is a Gaussian exponent, <= 0 and far above -100 wherever the result is used.
__device__ __forceinline__ float exp_neg(float x) {
    // x * log2(e) as an unevaluated sum ph + pl (compensated product); v_exp_f32 takes the rounded part
    // whole -- it does its own range reduction and x is a Gaussian exponent (<= 0, far above -100
    // wherever the result is used), so ocml's integer / fraction split, its ldexp and its range
    // selects are not needed -- and the residual enters to first order: 2^(ph+pl) = 2^ph (1 + pl ln 2).
    const float L2E_HI = __uint_as_float(0x3fb8aa3bu), L2E_LO = __uint_as_float(0x32a5705fu);
    const float LN2 = 0.6931471805599453f;
    float ph = x * L2E_HI;
    float pl = fmaf(x, L2E_HI, -ph);
    pl = fmaf(x, L2E_LO, pl);
    const float e = __builtin_amdgcn_exp2f(ph);
    return fmaf(e * pl, LN2, e);
}

// expf as glibc computes it (sysdeps/ieee754/flt-32/e_expf.c since 2.27: the ARM optimized-routines algorithm,
// restated from its published description): x N/ln2 = k + r with N = 32, 2^(k/N) from a 32-entry table of doubles,
// 2^(r/N) as a cubic, all in double, one rounding to float at the end.  On x86-64 glibc dispatches expf to a build
// compiled for FMA, where the compiler fused the reduction's r = z - kd with the product z = x N/ln2 (it enters
// unrounded); the polynomial's steps give the same float fused or not on the whole range.  This restates THAT build:
// with a rounded product one argument of the 1 118 699 521 in [-87, -0] (bits 0xc27c65d9, about -63.1) came out one
// unit below the host's expf, and the host's expf is what the oracle's frames hold.  Bit-identical to the host libm's expf --
// which is what the oracle (and, through Rust's f32::exp, the reference on a glibc host) calls -- on every input
// that can reach it here (every float in [-87, -0] on the device by tests/test_gpu_device_math.py, the host compile of
// this text by tests/test_device_math_host.py, a numpy restatement of the constants by tests/test_host.py).
// SPLAT_MODE_LIBM_EXP selects it: the frame is then the oracle's frame BIT FOR BIT, which shows that
// the exponential's last place is the only thing the default build rounds differently.  It costs ~18 double
// instructions per fragment, so it is a verification mode, not the default.
// tab[i] = bits(2^(i/32)) - (i << 47); one list, a device copy (staged in LDS by the compositor) and a host copy
#define SPLAT_EXP2F_TAB_LIST                                                                                              \
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull,  \
    0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull,  \
    0x3feedea64c123422ull, 0x3feece086061892dull, 0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull,  \
    0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,  \
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, 0x3feee89f995ad3adull,  \
    0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,  \
    0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull
__constant__ const unsigned long long EXP2F_TAB[32] = {SPLAT_EXP2F_TAB_LIST};
static constexpr unsigned long long EXP2F_TAB_HOST[32] = {SPLAT_EXP2F_TAB_LIST};
__host__ __device__ __forceinline__ float exp_libm(float x, const unsigned long long* __restrict__ tab /* LDS copy of EXP2F_TAB */) {
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0, SHIFT = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0, C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    // below -87 expf is < 2e-38 and the fragment is rejected for every opacity below 1 / (255 expf(-87)) ~ 2.4e35
    // (the precondition splat_upload_scene states); the clamp keeps k in the table's range without libm's underflow
    // branches, so the function returns expf(-87) there, not expf(x).  NaN stays NaN.
    const double xd = (double)((x != x) ? x : fmaxf(x, -87.0f));
    const double z = InvLn2N * xd;
    double kd = z + SHIFT;                                     // round to nearest integer, in the low mantissa bits
    const unsigned long long ki = __builtin_bit_cast(unsigned long long, kd);
    kd -= SHIFT;
    const double r = fma(InvLn2N, xd, -kd);                    // z - kd with the product unrounded: glibc's FMA build (see above)
    const double sc = __builtin_bit_cast(double, tab[ki & 31ull] + (ki << 47));
    const double zz = C0 * r + C1;
    const double r2 = r * r;
    double y = C2 * r + 1.0;
    y = zz * r2 + y;
    y = y * sc;
    return (float)y;
}

// glibc's expf for EVERY float (the PLY decoder's activations, splat_ply.hip: a log-scale or a logit is whatever the
// file holds).  The table, the cubic and the FMA-build reduction are exp_libm's, above; what is added is glibc's range
// handling: NaN stays NaN (x + x), above 0x1.62e42ep6 (log 2^128) the result is +inf, below -0x1.9fe368p6 (log 2^-150)
// it is +0, and in between nothing is special-cased -- a subnormal result is what the ONE rounding of the double to
// float gives, which needs float denormals on (the default of a HIP build).  The table is read where it lives: constant
// memory on the device (a load-time kernel, no LDS copy), the host copy on the host.  Bit-identical to the host libm's
// expf on every float in [-104, 89] (host compile: tests/test_ply_math_host.py) and on the patterns around every
// threshold plus a stride sweep of all 2^32 (device compile: tests/test_gpu_ply_device.py).
__host__ __device__ __forceinline__ float expf_libm_full(float x) {
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0, SHIFT = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0, C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long* const tab = EXP2F_TAB;
#else
    const unsigned long long* const tab = EXP2F_TAB_HOST;
#endif
    if (!(fabsf(x) < 88.0f)) {                                 // |x| >= 88, or NaN
        if (x != x) return x + x;
        if (x > 0x1.62e42ep6f) return __builtin_huge_valf();   // (+inf among them)
        if (x < -0x1.9fe368p6f) return 0.0f;                   // (-inf among them)
    }
    const double xd = (double)x;
    const double z = InvLn2N * xd;
    double kd = z + SHIFT;                                     // round to nearest integer, in the low mantissa bits
    const unsigned long long ki = __builtin_bit_cast(unsigned long long, kd);
    kd -= SHIFT;
    const double r = fma(InvLn2N, xd, -kd);                    // z - kd with the product unrounded: glibc's FMA build (see exp_libm)
    const double sc = __builtin_bit_cast(double, tab[ki & 31ull] + (ki << 47));
    const double zz = C0 * r + C1;
    const double r2 = r * r;
    double y = C2 * r + 1.0;
    y = zz * r2 + y;
    y = y * sc;
    return (float)y;
}
// the loader's sigmoid (src/gaussians.rs:267): IEEE operations around that expf, the divide correctly rounded
__host__ __device__ __forceinline__ float sigmoid_libm(float v) { return 1.0f / (1.0f + expf_libm_full(-v)); }

// k / 255.0f (IEEE) for every integer k in [0,255] in two instructions: 1/255 split into
// hi + lo floats, fma(k, hi, k*lo) rounds once (checked exhaustively in tests/test_host.py).
__host__ __device__ __forceinline__ float div255(float k) {
    const float RH = 0x1.010102p-8f, RL = -0x1.fdfdfep-33f;
    return fmaf(k, RH, k * RL);
}
// One channel of blend(): src/pipelines.rs:157-161.  Monotone non-decreasing in the state k for
// fixed alpha/colour (every step -- /255, *ia, +const, *255, clamp, trunc -- is monotone under
// round-to-nearest), which is what makes the [lo,hi] bracket of the early-out exact.
// The u8 cast saturates (NaN/negative -> 0, >= 255 -> 255).  Clamping the blended value to [0,1]
// BEFORE the *255 gives the same byte for every input (x in [0,1] is untouched; x > 1 -> 255; x < 0 or
// NaN -> 0) and folds into the add as its clamp modifier: one VALU less per channel than med3.
__device__ __forceinline__ float blend_channel(float k, float ia, float ac) {
    const float x = __builtin_amdgcn_fmed3f(ia * div255(k) + ac, 0.0f, 1.0f);
    return truncf(x * 255.0f);
}

// fragment(): src/pipelines.rs:134-143, branch-free.  (sx, sy) the sample (NaN off the target: never covered),
// a = (cx, cy, hx, hy), b = (A, B, C, opacity) with the y-axis sign folded into B by K1.  Returns alpha, forced to 0
// where the fragment is rejected or the sample is not covered; `cov` reports coverage.
template <class E>
__device__ __forceinline__ float fragment_alpha(float sx, float sy, const float4& a, const float4& b, E e_of_power, bool& cov) {
    float dx = sx - a.x, dy = a.y - sy;          // K1 folded the y-axis sign into b.y
    cov = (fabsf(dx) <= a.z) & (fabsf(dy) <= a.w);
    float power = -0.5f * (b.x * dx * dx + b.z * dy * dy) - b.y * dx * dy;
    float alpha = fminf(0.99f, b.w * e_of_power(power));
    bool accept = cov & !(power > 0.0f) & !(alpha < 1.0f / 255.0f);
    return accept ? alpha : 0.0f;
}

// ---- two records side by side (see the note on the paired walk in splat_kernels.hip) ----
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_add_clamp(f2 a, f2 b) {      // clamp(a + b, 0, 1) per component: the add's clamp modifier
    f2 r;                                                      // (NaN -> 0 like the one-record loop's v_add_f32 ... clamp)
    asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// blend() for two channels side by side: see blend_channel
__device__ __forceinline__ f2 blend_channel2(f2 k, float ia, f2 ac) {
    const float RH = 0x1.010102p-8f, RL = -0x1.fdfdfep-33f;
    const f2 f = __builtin_elementwise_fma(k, (f2)(RH), k * RL);       // div255, both channels
    const f2 y = pk_add_clamp(ia * f, ac) * 255.0f;
    return (f2){truncf(y.x), truncf(y.y)};
}
// exp_neg, both records
__device__ __forceinline__ f2 exp_neg2(f2 power) {
    const float L2E_HI = __uint_as_float(0x3fb8aa3bu), L2E_LO = __uint_as_float(0x32a5705fu), LN2 = 0.6931471805599453f;
    const f2 ph = power * L2E_HI;
    f2 pl = __builtin_elementwise_fma(power, (f2)(L2E_HI), -ph);
    pl = __builtin_elementwise_fma(power, (f2)(L2E_LO), pl);
    const f2 e = {__builtin_amdgcn_exp2f(ph.x), __builtin_amdgcn_exp2f(ph.y)};
    return __builtin_elementwise_fma(e * pl, (f2)(LN2), e);
}
// fragment() of two records (exp_neg): centres (cx, cy), half extents h = (hx0, hx1, hy0, hy1), conics (A, Bc, C) and
// opacities op, component 0 the first record.  Same operations per component, in the same order, as fragment_alpha.
__device__ __forceinline__ f2 fragment_alpha2(f2 sx2, f2 sy2, f2 cx, f2 cy, const float4& h, f2 A, f2 C, f2 Bc, f2 op) {
    const f2 dx = sx2 - cx, dy = cy - sy2;                     // K1 folded the y-axis sign into the cross term
    const bool cov0 = (fabsf(dx.x) <= h.x) & (fabsf(dy.x) <= h.z), cov1 = (fabsf(dx.y) <= h.y) & (fabsf(dy.y) <= h.w);
    const f2 power = -0.5f * (A * dx * dx + C * dy * dy) - Bc * dx * dy;
    const f2 ex = exp_neg2(power);
    const f2 al = op * ex;
    const float a0 = fminf(0.99f, al.x), a1 = fminf(0.99f, al.y);
    const float alpha0 = (cov0 & !(power.x > 0.0f) & !(a0 < 1.0f / 255.0f)) ? a0 : 0.0f;
    const float alpha1 = (cov1 & !(power.y > 0.0f) & !(a1 < 1.0f / 255.0f)) ? a1 : 0.0f;
    return (f2){alpha0, alpha1};
}
