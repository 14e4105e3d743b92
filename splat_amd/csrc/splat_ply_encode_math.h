// splat_ply_encode_math.h -- what ONE Gaussian of the resident scene looks like as a PLY row (splat_encode_ply_scene_device,
// splat_encode_ply_gaussians_device): the inverse of the loader's activations.  The scene holds a 3D covariance and an
// opacity; a PLY row holds the logs of three scales, a quaternion and a logit.  splat_ply_encode.hip includes this; so does
// tests/native/ply_encode_probe.hip, which runs it alone, compiled for the host and for the device
// (tests/test_ply_encode_math_host.py, tests/test_gpu_ply_encode.py).  Plain C++, __host__ __device__: one text for both.
//
// This header is the specification.  It calls nothing from libm -- no sqrt, no log, no fabs: every operation is an IEEE +, -,
// *, / or a comparison on doubles, or integer work on their bits -- and the translation units that include it are compiled
// with -ffp-contract=off, so the host compile and the device compile give the same bits by construction (the rule
// splat_sh_math.h and expf_libm_full follow).  Everything is computed in double and rounded to f32 ONCE, at the very end.
//
//   ply_eig3    S (symmetric 3x3, six f32) = V diag(lam) V^T: cyclic Jacobi, pairs (0,1) (0,2) (1,2), PLY_EIG_SWEEPS sweeps,
//               unrolled, scalars only (nothing is indexed at run time, so nothing goes to scratch).  A rotation whose
//               off-diagonal entry is exactly 0 is skipped.  V(r,c) = V[3c + r], columns are eigenvectors, det V = +1 (a
//               product of plane rotations; should the determinant come out negative, column 2 is negated).  The
//               eigenvalues are not sorted.
//   ply_log     0.5 ln(lam), the log of the SCALE whose square is lam.  lam <= 0 (a cov3d left zero, a rank-deficient
//               matrix, an eigenvalue rounding made negative): -104, whose expf is exactly 0 in the loader -- an absent
//               or zero scale.  NaN: NaN.
//   ply_logit   ln(o / (1 - o)).  o <= 0: -104 (sigmoid_libm gives exactly 0: a Gaussian deleted by opacity 0 stays
//               deleted); o >= 1: +104 (exactly 1); NaN: NaN; everything else is finite.
//   ply_quat    V -> the unit quaternion (i, j, k, w) the loader's compute_cov3d turns back into V: Shepperd's four
//               branches by the largest of trace, V00, V11, V22, in their division-free form, normalised; w >= 0, and
//               with w == 0 the first non-zero of i, j, k is positive.
//   ply_encode_one   the chain for one Gaussian: eight f32 in slot order (SPLAT_PLY_SLOT_SCALE .. SPLAT_PLY_SLOT_ROT + 3):
//               scale_0..2, opacity, rot_1 rot_2 rot_3 rot_0 = i j k w.
//
// Accuracy (tests/test_ply_encode_math_host.py, profiles/ply_save_accuracy.json): a covariance that goes through
// ply_encode_one and back through the loader (expf, normalisation, compute_cov3d in f32) returns within the error a float64
// numpy.linalg.eigh encoder leaves, class by class; the logs are within 1 ulp of the float64 ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int PLY_EIG_SWEEPS = 6;
constexpr float PLY_CLAMP = 104.0f;              // expf(-104) == 0 and 1 / (1 + expf(-104)) == 1 in f32, as the loader computes them

__host__ __device__ __forceinline__ uint64_t ply_bits(double x) { return __builtin_bit_cast(uint64_t, x); }
__host__ __device__ __forceinline__ double ply_from_bits(uint64_t b) { return __builtin_bit_cast(double, b); }
__host__ __device__ __forceinline__ float ply_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }

// sqrt of a positive normal double to within an ulp: x = m 4^h with m in [1, 4); (m + 2) / 3 is within 6 % of sqrt(m), and
// four Newton steps y <- (y + m / y) / 2 square that error four times.  Anything else in (NaN, inf) gives NaN or garbage,
// the same garbage on either side.
__host__ __device__ __forceinline__ double ply_sqrt(double x) {
    const uint64_t b = ply_bits(x);
    const int e = (int)((b >> 52) & 0x7ffu) - 1023;
    const int odd = e & 1;
    const double m = ply_from_bits((b & 0x800fffffffffffffull) | ((uint64_t)(1023 + odd) << 52));
    double y = (m + 2.0) / 3.0;
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    y = 0.5 * (y + m / y);
    return y * ply_from_bits((uint64_t)(1023 + ((e - odd) >> 1)) << 52);
}

// ln of a positive finite double (subnormals included), relative error below 1e-15: x = m 2^e with m in [sqrt 1/2, sqrt 2),
// s = (m - 1) / (m + 1), ln m = 2 s (1 + z / 3 + z^2 / 5 + ... + z^9 / 19) with z = s^2 <= 0.0295 (the first term dropped
// is below 2e-17), and e ln 2 added last -- with e == 0 nothing cancels, so the result is accurate near x == 1 as well.
__host__ __device__ __forceinline__ double ply_ln(double x) {
    int e = 0;
    if (x < 0x1p-1022) { x = x * 0x1p54; e = -54; }
    const uint64_t b = ply_bits(x);
    e += (int)((b >> 52) & 0x7ffu) - 1023;
    double m = ply_from_bits((b & 0x000fffffffffffffull) | (1023ull << 52));      // [1, 2)
    if (m > 0x1.6a09e667f3bcdp+0) { m = 0.5 * m; e += 1; }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    return (double)e * 0x1.62e42fefa39efp-1 + 2.0 * s * p;
}

__host__ __device__ __forceinline__ float ply_log(double lam) {
    if (lam != lam) return ply_nan();
    if (!(lam > 0.0)) return -PLY_CLAMP;
    if (!(lam < 0x1p1023)) return (float)lam;                  // (+inf, or a number whose log nobody will load again)
    return (float)(0.5 * ply_ln(lam));
}

__host__ __device__ __forceinline__ float ply_logit(float o) {
    if (o != o) return ply_nan();
    if (!(o > 0.0f)) return -PLY_CLAMP;
    if (!(o < 1.0f)) return PLY_CLAMP;
    const double d = (double)o;
    return (float)ply_ln(d / (1.0 - d));
}

// one Jacobi rotation in the plane (p, q): app aqq apq the pivot block, arp arq the third row's two entries, v?p v?q the two
// columns of V
__host__ __device__ __forceinline__ void ply_jacobi(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                                    double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    double t;
    if (at > 1e150) {
        t = 0.5 / theta;                                       // (theta^2 would overflow; the formula's limit)
    } else {
        t = 1.0 / (at + ply_sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / ply_sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y; arq = s * x + c * y;
    x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
    x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
    x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
}

// c6: S00 S01 S02 S11 S12 S22
__host__ __device__ __forceinline__ void ply_eig3(const float c6[6], double lam[3], double V[9]) {
    double a00 = (double)c6[0], a01 = (double)c6[1], a02 = (double)c6[2], a11 = (double)c6[3], a12 = (double)c6[4], a22 = (double)c6[5];
    double v00 = 1.0, v10 = 0.0, v20 = 0.0, v01 = 0.0, v11 = 1.0, v21 = 0.0, v02 = 0.0, v12 = 0.0, v22 = 1.0;   // v(row)(column)
#pragma unroll
    for (int sweep = 0; sweep < PLY_EIG_SWEEPS; ++sweep) {
        ply_jacobi(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        ply_jacobi(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        ply_jacobi(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    const double det = v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20) + v02 * (v10 * v21 - v11 * v20);
    if (det < 0.0) { v02 = -v02; v12 = -v12; v22 = -v22; }
    lam[0] = a00; lam[1] = a11; lam[2] = a22;
    V[0] = v00; V[1] = v10; V[2] = v20; V[3] = v01; V[4] = v11; V[5] = v21; V[6] = v02; V[7] = v12; V[8] = v22;
}

// q: i j k w
__host__ __device__ __forceinline__ void ply_quat(const double V[9], float q[4]) {
    const double m00 = V[0], m10 = V[1], m20 = V[2], m01 = V[3], m11 = V[4], m21 = V[5], m02 = V[6], m12 = V[7], m22 = V[8];
    const double tr = m00 + m11 + m22;
    double w, i, j, k;
    if (tr >= m00 && tr >= m11 && tr >= m22) {
        w = 1.0 + tr; i = m21 - m12; j = m02 - m20; k = m10 - m01;
    } else if (m00 >= m11 && m00 >= m22) {
        w = m21 - m12; i = ((1.0 + m00) - m11) - m22; j = m01 + m10; k = m02 + m20;
    } else if (m11 >= m22) {
        w = m02 - m20; i = m01 + m10; j = ((1.0 + m11) - m00) - m22; k = m12 + m21;
    } else {
        w = m10 - m01; i = m02 + m20; j = m12 + m21; k = ((1.0 + m22) - m00) - m11;
    }
    const double inv = 1.0 / ply_sqrt(((w * w + i * i) + j * j) + k * k);
    w = w * inv; i = i * inv; j = j * inv; k = k * inv;
    const bool flip = w < 0.0 || (w == 0.0 && (i < 0.0 || (i == 0.0 && (j < 0.0 || (j == 0.0 && k < 0.0)))));
    if (flip) { w = -w; i = -i; j = -j; k = -k; }
    q[0] = (float)i; q[1] = (float)j; q[2] = (float)k; q[3] = (float)w;
}

// cov: the nine floats of the scene, S(r,c) = cov[3c + r]; the upper triangle is read.  out: scale_0 scale_1 scale_2 opacity
// rot_1 rot_2 rot_3 rot_0
__host__ __device__ __forceinline__ void ply_encode_one(const float cov[9], float opacity, float out[8]) {
    const float c6[6] = {cov[0], cov[3], cov[6], cov[4], cov[7], cov[8]};
    double lam[3], V[9];
    ply_eig3(c6, lam, V);
    out[0] = ply_log(lam[0]); out[1] = ply_log(lam[1]); out[2] = ply_log(lam[2]);
    out[3] = ply_logit(opacity);
    ply_quat(V, out + 4);
}
