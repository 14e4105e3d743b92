// splat_colour_math.h -- the colour ONE Gaussian of the resident scene is drawn with under a camera, a test on that colour,
// and a 3x4 map applied to it where it is kept: in the sh coefficients (splat_eval_colours_device,
// splat_select_colour_device, splat_recolour_scene_device, splat_recolour_gaussians_device).  splat_colour.hip includes it;
// so does tests/native/colour_math_probe.hip, which runs it alone, compiled for the host and for the device
// (tests/test_colour_math_host.py, tests/test_gpu_colour.py).  Plain C++; what is applied per Gaussian is
// __host__ __device__: one text for both.  Every product, sum, quotient and root is rounded to f32 once, in the order
// written -- the translation units that include this are compiled with -ffp-contract=off, and the formulas rest on it.
//
// colour_under_camera is the colour half of K1 (preprocess_kernel of splat_kernels.hip, "ray_direction ...
// eval_spherical_harmonics ... + 0.5f") restated: the same f32 operations in the same order, so the same bits -- the rgb of
// the record a frame of that camera is made of, for every Gaussian, visible or not.  K1's replacement of a non-finite colour
// by +-FLT_MAX is blending's business and is not part of it: a NaN stays a NaN.
//
// A channel's 16 coefficients lie at sh[3k + ch], in four bands: k = 0 | 1..3 | 4..8 | 9..15.  The colour is linear in them,
//   eval_sh(sh, d) = C0 sh_0 + sum_{k >= 1} Y_k(d) sh_k + 0.5        (per channel)
// so a map rgb' = A rgb + t of the colour is a map of the coefficients: every sh_k becomes A sh_k, and band 0 -- the only
// one that carries a constant -- takes the offset o = (t + 0.5 (A 1) - 0.5) / C0 on top.  In exact arithmetic
// eval_sh(sh', d) = A eval_sh(sh, d) + t then holds for every direction and every sh_dim, band 0 alone included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/splat_hip.h"

struct SplatColourMap { float a[9]; float o[3]; };   // A row-major, a[3i+k] = A(i,k); o: band 0's offset (a kernel argument by value: SGPRs)

// the basis constants, src/gaussians.rs:11-26 (SH_C* of splat_kernels.hip)
namespace splat_colour {
constexpr float C0 = 0.28209479177387814f;
constexpr float C1 = 0.4886025119029199f;
constexpr float C2_0 = 1.0925484305920792f, C2_1 = -1.0925484305920792f, C2_2 = 0.31539156525252005f, C2_3 = -1.0925484305920792f,
                C2_4 = 0.5462742152960396f;
constexpr float C3_0 = -0.5900435899266435f, C3_1 = 2.890611442640554f, C3_2 = -0.4570457994644658f, C3_3 = 0.3731763325901154f,
                C3_4 = -0.4570457994644658f, C3_5 = 1.445305721320277f, C3_6 = -0.5900435899266435f;
}  // namespace splat_colour

// ---- one Gaussian, on either side ---------------------------------------------------------------------------------------
// p: the centre; sh: the 48 floats, of which only those of the bands sh_dim names are read (band 0 always, band 1 with
// sh_dim > 3, band 2 with > 12, band 3 with > 27).  A Gaussian AT the camera has a 0 / 0 direction: NaN from band 1 on.
__host__ __device__ __forceinline__ void colour_under_camera(const float p[3], const float cam_pos[3], int sh_dim, const float* sh,
                                                             float rgb[3]) {
    using namespace splat_colour;
    const float dxw = p[0] - cam_pos[0], dyw = p[1] - cam_pos[1], dzw = p[2] - cam_pos[2];
    const float nrm = sqrtf((dxw * dxw + dyw * dyw) + dzw * dzw);
    const float x = dxw / nrm, y = dyw / nrm, z = dzw / nrm;
    float col[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) col[ch] = C0 * sh[ch];
    if (sh_dim > 3) {
        const float k1 = C1 * y, k2 = C1 * z, k3 = C1 * x;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) col[ch] = col[ch] - k1 * sh[3 + ch] + k2 * sh[6 + ch] - k3 * sh[9 + ch];
        if (sh_dim > 12) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            const float k4 = C2_0 * xy, k5 = C2_1 * yz, k6 = C2_2 * (2.0f * zz - xx - yy);
            const float k7 = C2_3 * xz, k8 = C2_4 * (xx - yy);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                col[ch] = col[ch] + k4 * sh[12 + ch] + k5 * sh[15 + ch] + k6 * sh[18 + ch] + k7 * sh[21 + ch] + k8 * sh[24 + ch];
            if (sh_dim > 27) {
                const float k9 = C3_0 * y * (3.0f * xx - yy), k10 = C3_1 * xy * z;
                const float k11 = C3_2 * y * (4.0f * zz - xx - yy);
                const float k12 = C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
                const float k13 = C3_4 * x * (4.0f * zz - xx - yy), k14 = C3_5 * z * (xx - yy);
                const float k15 = C3_6 * x * (xx - 3.0f * yy);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    col[ch] = col[ch] + k9 * sh[27 + ch] + k10 * sh[30 + ch] + k11 * sh[33 + ch] + k12 * sh[36 + ch] +
                              k13 * sh[39 + ch] + k14 * sh[42 + ch] + k15 * sh[45 + ch];
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = col[ch] + 0.5f;   // HALF, no clamp
}

// The VOLUME test of splat_select_query in colour space: u = colour_to_unit (rgb 1), inside the unit box or the unit ball.
// clamp: each channel first to [0, 1], by comparisons that leave a NaN a NaN (fmaxf would turn it into 0).  A NaN fails.
__host__ __device__ __forceinline__ bool colour_passes(const splat_colour_query& q, const float rgb[3]) {
    float c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float v = rgb[ch];
        c[ch] = q.clamp != 0u ? (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)) : v;
    }
    const float* m = q.colour_to_unit;
    float u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = ((m[4 * k] * c[0] + m[4 * k + 1] * c[1]) + m[4 * k + 2] * c[2]) + m[4 * k + 3];
    if (q.shape == 0u) return (fabsf(u[0]) <= 1.0f) && (fabsf(u[1]) <= 1.0f) && (fabsf(u[2]) <= 1.0f);
    return ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) <= 1.0f;
}

// sh: the 48 floats of a Gaussian, in place.  The three channels of a coefficient are read before any of them is written.
// Nothing is checked: with a non-finite coefficient 0 * inf is NaN, so one inf or NaN makes all three channels of its
// coefficient NaN, also under the identity.
__host__ __device__ __forceinline__ void recolour_coefficients(const SplatColourMap& m, float sh[48]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float r = sh[3 * k], g = sh[3 * k + 1], b = sh[3 * k + 2];
        const float v0 = (m.a[0] * r + m.a[1] * g) + m.a[2] * b;
        const float v1 = (m.a[3] * r + m.a[4] * g) + m.a[5] * b;
        const float v2 = (m.a[6] * r + m.a[7] * g) + m.a[8] * b;
        sh[3 * k] = k == 0 ? v0 + m.o[0] : v0;
        sh[3 * k + 1] = k == 0 ? v1 + m.o[1] : v1;
        sh[3 * k + 2] = k == 0 ? v2 + m.o[2] : v2;
    }
}

// ---- the map: host only, double ------------------------------------------------------------------------------------------
// m: 3x4 row-major, rgb' = A rgb + t with A(i,k) = m[4i+k], t_i = m[4i+3].  o_i = (t_i + 0.5 ((A_i0 + A_i1) + A_i2) - 0.5) / C0,
// in double from the f32 entries, C0 being the f32 constant widened; rounded to f32 once.
inline void recolour_offset(const float m[12], float o[3]) {
    const double c0 = (double)splat_colour::C0;
    for (int i = 0; i < 3; ++i) {
        const double row = ((double)m[4 * i] + (double)m[4 * i + 1]) + (double)m[4 * i + 2];
        o[i] = (float)(((double)m[4 * i + 3] + 0.5 * row - 0.5) / c0);
    }
}

// what the recolour entry points refuse in m; nullptr: nothing.  out: the map as the kernels take it.
inline const char* recolour_map(const float m[12], SplatColourMap& out) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(m[i])) return "m: a non-finite entry";
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) out.a[3 * i + k] = m[4 * i + k];
    recolour_offset(m, out.o);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(out.o[i])) return "m: the offset of band 0, (t + 0.5 (A 1) - 0.5) / C0, is not finite in f32";
    return nullptr;
}
