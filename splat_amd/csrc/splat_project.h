// splat_project.h -- the geometry half of the vertex stage for one Gaussian, written once for the scene queries that restate
// it: the selection (splat_select.hip) and the pick (splat_pick.hip).  It is K1's (preprocess_kernel of splat_kernels.hip):
// the same f32 operations in the same order (project_cov3d_to_screen, the conic, the half extents, NDC to pixels, visibility,
// covered_interval), and both files are built with K1's flags -- no contraction, correctly rounded division and square root --
// so the same bits (tests/test_gpu_select.py and tests/test_gpu_pick.py hold them to the oracle).  Device code only.
#pragma once
#include "splat_internal.h"

namespace splat {

// ---------------------------------------------------------------------------
// K1's small helpers, as splat_kernels.hip has them (column-major; products accumulate left to right)
// ---------------------------------------------------------------------------
struct SelMat3 { float m[9]; };
#define SM3(A, r, c) ((A).m[(c) * 3 + (r)])

static __device__ __forceinline__ SelMat3 sel_mat3_mul(const SelMat3& a, const SelMat3& b) {
    SelMat3 c;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float acc = SM3(a, i, 0) * SM3(b, 0, j);
            acc = SM3(a, i, 1) * SM3(b, 1, j) + acc;
            acc = SM3(a, i, 2) * SM3(b, 2, j) + acc;
            SM3(c, i, j) = acc;
        }
    return c;
}
static __device__ __forceinline__ SelMat3 sel_mat3_t(const SelMat3& a) {
    SelMat3 t;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) SM3(t, i, j) = SM3(a, j, i);
    return t;
}
// row i of m * (x, y, z, w)
static __device__ __forceinline__ float sel_mat4_row(const float* m, int i, float x, float y, float z, float w) {
    float acc = m[0 + i] * x;
    acc = m[4 + i] * y + acc;
    acc = m[8 + i] * z + acc;
    acc = m[12 + i] * w + acc;
    return acc;
}
static __device__ __forceinline__ bool sel_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// Exactly covered pixel interval {p in [lo_lim,hi_lim] : |p + off - c| <= h}; false when empty.
static __device__ __forceinline__ bool sel_covered_interval(float c, float h, float off, int lo_lim, int hi_lim, int* lo, int* hi) {
    float flo = c - h - off, fhi = c + h - off;
    if (!(fhi >= (float)lo_lim - 2.0f) || !(flo <= (float)hi_lim + 2.0f)) return false;
    int a = (int)fmaxf(floorf(flo) - 1.0f, (float)lo_lim);
    int b = (int)fminf(ceilf(fhi) + 1.0f, (float)hi_lim);
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    while (a <= b && !(fabsf(((float)a + off) - c) <= h)) ++a;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    while (b >= a && !(fabsf(((float)b + off) - c) <= h)) --b;
    if (a > b) return false;
    *lo = a; *hi = b;
    return true;
}

// The geometry half of the vertex stage for one Gaussian: centre, and the covered pixel range when it is visible on the
// whole target (K1's `on_target`, the oracle's `visible`).  pc2 = view-space z (splat_record.depth).
// more (nullable): the rest of the record a fragment is evaluated with -- the conic, the half extents and the view-space z.
// A NaN z is never visible: it enters q[2] through proj[10] * pc[2], so ndcz is NaN and fails sel_finite.
struct SelProjected { float ca, cb, cc, hx, hy, z; };
template <bool CORRECTED>
static __device__ __forceinline__ bool sel_project(const SelectView& fc, float px, float py, float pz, const float (&c9)[9],
                                                   float* cx_out, float* cy_out, int (&r)[4], SelProjected* more = nullptr) {
    // project_cov3d_to_screen                                            src/gaussians.rs:114-161
    float pc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pc[i] = sel_mat4_row(fc.view, i, px, py, pz, 1.0f);
    float limx = 1.3f * fc.htanx, limy = 1.3f * fc.htany;
    float txtz = pc[0] / pc[2], tytz = pc[1] / pc[2];
    float tx = fminf(limx, fmaxf(-limx, txtz)) * pc[2];
    float ty = fminf(limy, fmaxf(-limy, tytz)) * pc[2];
    float tz = pc[2];
    SelMat3 J;
    SM3(J, 0, 0) = fc.focal / tz; SM3(J, 0, 1) = 0.0f;          SM3(J, 0, 2) = -(fc.focal * tx) / (tz * tz);
    SM3(J, 1, 0) = 0.0f;          SM3(J, 1, 1) = fc.focal / tz; SM3(J, 1, 2) = -(fc.focal * ty) / (tz * tz);
    SM3(J, 2, 0) = 0.0f;          SM3(J, 2, 1) = 0.0f;          SM3(J, 2, 2) = 0.0f;
    SelMat3 Wm;   // viewmatrix.fixed_view::<3,3>(0,0).transpose()
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) SM3(Wm, a, b) = fc.view[a * 4 + b];
    SelMat3 T = CORRECTED ? sel_mat3_mul(Wm, sel_mat3_t(J)) : sel_mat3_mul(Wm, J);
    SelMat3 Sg;
#pragma unroll
    for (int e = 0; e < 9; ++e) Sg.m[e] = c9[e];
    SelMat3 cov = sel_mat3_mul(sel_mat3_mul(sel_mat3_t(T), sel_mat3_t(Sg)), T);
    float m11 = SM3(cov, 0, 0) + fc.lowpass, m21 = SM3(cov, 1, 0), m12 = SM3(cov, 0, 1), m22 = SM3(cov, 1, 1) + fc.lowpass;

    // gaussian_vertex_shader                                             src/pipelines.rs:17-51
    float det = m11 * m22 - m21 * m12;
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = sel_mat4_row(fc.proj, i, pc[0], pc[1], pc[2], pc[3]);
    float ndcx = q[0] / q[3], ndcy = q[1] / q[3], ndcz = q[2] / q[3];
    float ca = m22 / det, cb = -m12 / det, cc = m11 / det;
    float hx = 3.0f * sqrtf(m11), hy = 3.0f * sqrtf(m22);
    // euc: NDC -> target pixels
    float cx = (ndcx * 0.5f + 0.5f) * fc.w;
    float cy = fc.y_up ? (ndcy * -0.5f + 0.5f) * fc.h : (ndcy * 0.5f + 0.5f) * fc.h;
    bool vis = !(det == 0.0f) && sel_finite(cx) && sel_finite(cy) && sel_finite(hx) && sel_finite(hy) && sel_finite(ca) &&
               sel_finite(cb) && sel_finite(cc) && sel_finite(ndcz);
    if (vis && fc.zclip) vis = (fc.zmin <= ndcz) && (ndcz <= fc.zmax);
    const float off = fc.sample_half ? 0.5f : 0.0f;
    *cx_out = cx; *cy_out = cy;
    if (more) { more->ca = ca; more->cb = cb; more->cc = cc; more->hx = hx; more->hy = hy; more->z = pc[2]; }
    return vis && sel_covered_interval(cx, hx, off, 0, fc.W - 1, &r[0], &r[1]) &&
           sel_covered_interval(cy, hy, off, 0, fc.H - 1, &r[2], &r[3]);
}

}  // namespace splat
