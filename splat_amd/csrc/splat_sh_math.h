// splat_sh_math.h -- what an orthogonal map R (world -> world) does to the view-dependent colour of ONE Gaussian of the
// resident scene (splat_rotate_sh_scene_device, splat_rotate_sh_gaussians_device, splat_sh_rotation_blocks): the sh
// coefficients turn with the scene, so that eval_sh(c', R d) == eval_sh(c, d) for every unit d.  splat_transform.hip
// includes it; so does tests/native/sh_rotate_probe.hip, which runs it alone, compiled for the host and for the device
// (tests/test_sh_rotate_math_host.py, tests/test_gpu_sh_rotate.py).  Plain C++; the part applied per Gaussian is
// __host__ __device__: one text for both.
//
// A channel's 16 coefficients lie at sh[3k + ch], in four bands: k = 0 | 1..3 | 4..8 | 9..15.  Band 0 is constant over the
// sphere and keeps its bits; band l (n = 2l+1 coefficients) is multiplied by an n x n block D_l(R):
//   c'_m = (((D(m,0) c_0 + D(m,1) c_1) + D(m,2) c_2) + ...) + D(m,n-1) c_{n-1}
// summed left to right, every product and every sum rounded to f32 once -- the translation units that include this are
// compiled with -ffp-contract=off, and the formula rests on it.  Every input of a band is read before any of its outputs is
// written.  Nothing is checked: with a non-finite coefficient 0 * inf is NaN, so one inf or NaN in a band makes the whole
// band of that channel NaN, also under the identity.
//
// The blocks (host only, double) come from eval_sh's own fifteen polynomials and f32 constants, restated below -- this
// basis has its own signs and order, so no textbook Wigner matrix is taken over.  With B_l(i,m) the m-th function of band l
// at direction d_i and B_l^R(i,m) the same at R^T d_i, D_l is the least-squares solution of B_l D_l = B_l^R over 32 fixed
// directions on a Fibonacci spiral (z_i = 1 - (2i+1)/32, phi_i = (i + 0.5) pi (3 - sqrt 5)): normal equations, plain
// elimination (cond B_l < 1.15).  Every entry is then snapped to the nearest multiple of 2^-40 -- at most 4.6e-13, five
// orders below f32 roundoff, which turns solver noise into exact zeros and exact +-1 -- and rounded to f32.  The identity,
// the axis-aligned quarter turns and the axis mirrors therefore give exact signed permutations: four quarter turns return
// every non-zero coefficient's bits (a zero stays a zero; its sign is the sum's).  Reflections (det = -1) are served like
// rotations.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

struct SplatShBlocks { float d1[9], d2[25], d3[49]; };   // row-major, d_l[(2l+1) m + k] = D_l(m,k); 83 floats (a kernel argument by value: SGPRs)

// ---- one Gaussian, on either side ---------------------------------------------------------------------------------------
// c: the band's 3n floats, c[3m + ch]
template <int N>
__host__ __device__ __forceinline__ void rotate_sh_band(const float* D, float* c) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float in[N];
#pragma unroll
        for (int k = 0; k < N; ++k) in[k] = c[3 * k + ch];
#pragma unroll
        for (int m = 0; m < N; ++m) {
            float a = D[N * m] * in[0];
#pragma unroll
            for (int k = 1; k < N; ++k) a = a + D[N * m + k] * in[k];
            c[3 * m + ch] = a;
        }
    }
}

// sh45: the floats sh[3..48) of a Gaussian, in place
__host__ __device__ __forceinline__ void rotate_sh_bands(const SplatShBlocks& b, float sh45[45]) {
    rotate_sh_band<3>(b.d1, sh45);
    rotate_sh_band<5>(b.d2, sh45 + 9);
    rotate_sh_band<7>(b.d3, sh45 + 24);
}

// ---- the blocks: host only, double --------------------------------------------------------------------------------------
// the 15 functions of bands 1-3 at (x, y, z), as eval_sh weighs sh[3k..3k+3), k = 1..15: y[k-1]
inline void sh_basis_bands(double x, double y, double z, double out[15]) {
    const double C1 = (double)0.4886025119029199f;
    const double C2[5] = {(double)1.0925484305920792f, (double)-1.0925484305920792f, (double)0.31539156525252005f,
                          (double)-1.0925484305920792f, (double)0.5462742152960396f};
    const double C3[7] = {(double)-0.5900435899266435f, (double)2.890611442640554f, (double)-0.4570457994644658f,
                          (double)0.3731763325901154f, (double)-0.4570457994644658f, (double)1.445305721320277f,
                          (double)-0.5900435899266435f};
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    out[0] = -C1 * y;
    out[1] = C1 * z;
    out[2] = -C1 * x;
    out[3] = C2[0] * xy;
    out[4] = C2[1] * yz;
    out[5] = C2[2] * (2.0 * zz - xx - yy);
    out[6] = C2[3] * xz;
    out[7] = C2[4] * (xx - yy);
    out[8] = C3[0] * y * (3.0 * xx - yy);
    out[9] = C3[1] * xy * z;
    out[10] = C3[2] * y * (4.0 * zz - xx - yy);
    out[11] = C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
    out[12] = C3[4] * x * (4.0 * zz - xx - yy);
    out[13] = C3[5] * z * (xx - yy);
    out[14] = C3[6] * x * (xx - 3.0 * yy);
}

// what the entry points refuse in r (3x3 row-major, f32 entries judged in double); nullptr: nothing
inline const char* sh_rotation_refusal(const float r[9]) {
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(r[i])) return "a non-finite entry in r";
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += (double)r[3 * i + k] * (double)r[3 * j + k];
            if (!(std::fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-4)) return "r is not orthogonal (max |R R^T - I| > 1e-4)";
        }
    return nullptr;
}

// D (N x N, row-major) from the N columns at `first` of the 32 x 15 tables B and BR: (B^T B) D = B^T BR
template <int N>
inline void sh_solve_block(const double B[32][15], const double BR[32][15], int first, float* D) {
    double A[N][2 * N];                          // [B^T B | B^T BR]
    for (int m = 0; m < N; ++m)
        for (int k = 0; k < N; ++k) {
            double g = 0.0, h = 0.0;
            for (int i = 0; i < 32; ++i) { g += B[i][first + m] * B[i][first + k]; h += B[i][first + m] * BR[i][first + k]; }
            A[m][k] = g; A[m][N + k] = h;
        }
    for (int p = 0; p < N; ++p) {                // Gauss-Jordan; B^T B is positive definite and well conditioned: no pivoting
        const double inv = 1.0 / A[p][p];
        for (int k = 0; k < 2 * N; ++k) A[p][k] *= inv;
        for (int m = 0; m < N; ++m) {
            if (m == p) continue;
            const double f = A[m][p];
            for (int k = 0; k < 2 * N; ++k) A[m][k] -= f * A[p][k];
        }
    }
    const double SNAP = 1099511627776.0;         // 2^40
    for (int m = 0; m < N; ++m)
        for (int k = 0; k < N; ++k) D[N * m + k] = (float)(std::rint(A[m][N + k] * SNAP) / SNAP);
}

// the three blocks of r; r arrives judged (sh_rotation_refusal)
inline void sh_rotation_blocks(const float r[9], SplatShBlocks& out) {
    static const double PI = 3.14159265358979323846;
    double B[32][15], BR[32][15];
    for (int i = 0; i < 32; ++i) {
        const double z = 1.0 - (2.0 * i + 1.0) / 32.0, phi = (i + 0.5) * PI * (3.0 - std::sqrt(5.0));
        const double s = std::sqrt(1.0 - z * z), x = s * std::cos(phi), y = s * std::sin(phi);
        sh_basis_bands(x, y, z, B[i]);
        // R^T d
        sh_basis_bands((double)r[0] * x + (double)r[3] * y + (double)r[6] * z, (double)r[1] * x + (double)r[4] * y + (double)r[7] * z,
                       (double)r[2] * x + (double)r[5] * y + (double)r[8] * z, BR[i]);
    }
    sh_solve_block<3>(B, BR, 0, out.d1);
    sh_solve_block<5>(B, BR, 3, out.d2);
    sh_solve_block<7>(B, BR, 8, out.d3);
}
