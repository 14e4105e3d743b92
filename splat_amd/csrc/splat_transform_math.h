// splat_transform_math.h -- what an affine map does to ONE Gaussian of the resident scene (splat_transform_scene_device,
// splat_transform_gaussians_device): the centre and the 3D covariance.  splat_transform.hip includes it; so does
// tests/native/transform_math_probe.hip, which runs it alone, compiled for the host and for the device
// (tests/test_transform_math_host.py, tests/test_gpu_scene_read.py).  Plain C++, __host__ __device__: one text for both.
//
// m: 3x4 row-major, A(r,k) = m[4r+k], translation m[4r+3].  cov: a column-major 3x3 block, S(r,c) = cov[3c+r].
// Every product and every sum is rounded to f32 once, in the order written -- the translation units that include this
// are compiled with -ffp-contract=off, and the formulas rest on it:
//   p'_r    = ((A(r,0) x + A(r,1) y) + A(r,2) z) + m[4r+3]
//   T(r,c)  =  (A(r,0) S(0,c) + A(r,1) S(1,c)) + A(r,2) S(2,c)            T = A S
//   S'(r,c) =  (T(r,0) A(c,0) + T(r,1) A(c,1)) + T(r,2) A(c,2)            S' = T A^T, all nine, each on its own
// Nothing is symmetrised and nothing is checked: any float may stand in m.
#pragma once
#include <hip/hip_runtime.h>

struct SplatAffine { float m[12]; };             // (a kernel argument by value: it lives in SGPRs)

__host__ __device__ __forceinline__ void transform_point(const float* m, float x, float y, float z, float out[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

__host__ __device__ __forceinline__ void transform_cov3d(const float* m, const float cov[9], float out[9]) {
    float T[3][3];                               // T[r][c]
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            T[r][c] = (m[4 * r] * cov[3 * c] + m[4 * r + 1] * cov[3 * c + 1]) + m[4 * r + 2] * cov[3 * c + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            out[3 * c + r] = (T[r][0] * m[4 * c] + T[r][1] * m[4 * c + 1]) + T[r][2] * m[4 * c + 2];
}
