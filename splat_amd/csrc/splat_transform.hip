// splat_transform.hip -- the resident scene read back and mapped where it lies (splat_read_scene_device,
// splat_read_gaussians_device, splat_transform_scene_device, splat_transform_gaussians_device, splat_rotate_sh_scene_device,
// splat_rotate_sh_gaussians_device; gfx950).
//
//   unpack_kernel<INDEXED>      the named fields' float slots of the planes into the caller's buffers: repack_kernel of
//                               splat_update.hip run backwards, with the same slot map
//   transform_kernel<INDEXED>   an affine map applied to the centre and the 3D covariance of a Gaussian, in place on the
//                               planes (splat_transform_math.h); opacity and sh keep their bits
//   rotate_sh_kernel<INDEXED>   bands 1-3 of the sh coefficients of a Gaussian turned by an orthogonal map, in place on the
//                               planes (splat_sh_math.h); everything else keeps its bits
//
// All three are memory bound and need no LDS.  The order of the scene (orig[]) stays, as under every edit; the inverse of the
// order, the index check and the bounds from the planes are splat_update.hip's.
#include "splat_internal.h"
#include "splat_transform_math.h"
#include "splat_sh_math.h"

namespace splat {

// ---------------------------------------------------------------------------
// Unpack.  Float slots of a Gaussian as pack_scene_kernel lays them out: 0-2 xyz, 3 opacity, 4-12 cov3d, 13-60 sh; plane p
// holds slots 4p .. 4p+3.  The planes hold the caller's very floats, so what comes back is what went in, bit for bit; the
// w of pos4, which the planes do not store, comes back as 1.  A buffer whose field is not named is not touched.
// INDEXED = false: thread j reads slot j (float4 loads, coalesced) and writes row orig[j] of the caller's buffers (rows == n).
// INDEXED = true:  thread t reads slot inv[index[t]] and writes row t of the COMPACT buffers (rows == k); an index named
// twice is read twice, into two rows.
// (51 VGPRs as it stands: repack_kernel's amdgpu_waves_per_eu(8) is not needed here -- the stores drain the sh planes as they arrive)
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(256)
void unpack_kernel(uint64_t n, uint64_t rows, uint32_t fields, float* __restrict__ pos4, float* __restrict__ cov3d,
                   float* __restrict__ opacity, float* __restrict__ sh, const unsigned int* __restrict__ orig,
                   const unsigned int* __restrict__ index, const unsigned int* __restrict__ inv,
                   const float4* __restrict__ planes) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= rows) return;
    uint64_t j, r;                                             // the slot read, the row written
    if (INDEXED) { r = t; j = inv[index[t]]; } else { j = t; r = orig[t]; }
    const bool f_pos = fields & SPLAT_FIELD_POS, f_cov = fields & SPLAT_FIELD_COV3D, f_op = fields & SPLAT_FIELD_OPACITY,
               f_sh = fields & SPLAT_FIELD_SH;
    if (f_pos || f_op) {
        const float4 v = planes[j];
        if (f_pos) { pos4[4 * r] = v.x; pos4[4 * r + 1] = v.y; pos4[4 * r + 2] = v.z; pos4[4 * r + 3] = 1.0f; }
        if (f_op) opacity[r] = v.w;
    }
    if (f_cov) {
        const float4 c0 = planes[n + j], c1 = planes[2 * n + j];
        float* c = cov3d + 9 * r;
        c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w;
        c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
    }
    if (f_cov || f_sh) {
        const float4 v = planes[3 * n + j];
        if (f_cov) cov3d[9 * r + 8] = v.x;
        if (f_sh) { sh[48 * r] = v.y; sh[48 * r + 1] = v.z; sh[48 * r + 2] = v.w; }
    }
    if (f_sh) {
        float* q = sh + 48 * r + 3;                            // plane p, 4 <= p <= 14: sh[4p - 13 .. 4p - 10]
#pragma unroll
        for (int p = 4; p < 15; ++p, q += 4) {
            const float4 v = planes[(uint64_t)p * n + j];
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        }
        q[0] = planes[15 * n + j].x;                           // sh[47]
    }
}

// ---------------------------------------------------------------------------
// Transform.  Planes 0-3 of slot j hold x y z | opacity, cov[0..3], cov[4..7], cov[8] | sh0 sh1 sh2: four float4 loads, the
// map of splat_transform_math.h, four float4 stores -- 128 bytes a Gaussian.  Opacity and the three sh floats go back as they
// came.  A slot belongs to one thread (the indices are distinct), so nothing races.
// INDEXED = false: thread j maps slot j (rows == n).
// INDEXED = true:  thread t maps slot inv[index[t]] (rows == k) and marks the slot's block dirty: a plain byte store of 1,
// the same value from every thread that stores it.
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(256)
void transform_kernel(uint64_t n, uint64_t rows, SplatAffine a, const unsigned int* __restrict__ index,
                      const unsigned int* __restrict__ inv, float4* __restrict__ planes, unsigned char* __restrict__ dirty) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= rows) return;
    const uint64_t j = INDEXED ? (uint64_t)inv[index[t]] : t;
    float4 p0 = planes[j], p1 = planes[n + j], p2 = planes[2 * n + j], p3 = planes[3 * n + j];
    const float cov[9] = {p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w, p3.x};
    float pos[3], out[9];
    transform_point(a.m, p0.x, p0.y, p0.z, pos);
    transform_cov3d(a.m, cov, out);
    p0.x = pos[0]; p0.y = pos[1]; p0.z = pos[2];
    p3.x = out[8];
    planes[j] = p0;
    planes[n + j] = make_float4(out[0], out[1], out[2], out[3]);
    planes[2 * n + j] = make_float4(out[4], out[5], out[6], out[7]);
    planes[3 * n + j] = p3;
    if (INDEXED) dirty[j >> 8] = (unsigned char)1;
}

// ---------------------------------------------------------------------------
// Rotate sh.  sh[3..48) of slot j lies in planes 4-14 (plane p: sh[4p - 13 .. 4p - 10]) and in plane 15's .x (sh[47]): twelve
// float4 loads, the three band products of splat_sh_math.h (249 multiply-adds), twelve float4 stores -- 384 bytes a Gaussian.
// Plane 3 (cov[8] and band 0) is not touched; plane 15's .yzw go back as they came.  Every index into the 45 values is a
// constant after unrolling, so they live in registers; the 83 block floats are a by-value argument.  Positions and
// covariances stay, so no block bounds change and nothing is marked dirty.
// INDEXED = false: thread j maps slot j (rows == n).  INDEXED = true: thread t maps slot inv[index[t]] (rows == k).
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(256)
void rotate_sh_kernel(uint64_t n, uint64_t rows, SplatShBlocks b, const unsigned int* __restrict__ index,
                      const unsigned int* __restrict__ inv, float4* __restrict__ planes) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= rows) return;
    const uint64_t j = INDEXED ? (uint64_t)inv[index[t]] : t;
    float4 v[12];
#pragma unroll
    for (int p = 0; p < 12; ++p) v[p] = planes[(uint64_t)(p + 4) * n + j];
    float c[45];
#pragma unroll
    for (int p = 0; p < 11; ++p) { c[4 * p] = v[p].x; c[4 * p + 1] = v[p].y; c[4 * p + 2] = v[p].z; c[4 * p + 3] = v[p].w; }
    c[44] = v[11].x;
    rotate_sh_bands(b, c);
#pragma unroll
    for (int p = 0; p < 11; ++p) planes[(uint64_t)(p + 4) * n + j] = make_float4(c[4 * p], c[4 * p + 1], c[4 * p + 2], c[4 * p + 3]);
    v[11].x = c[44];
    planes[15 * n + j] = v[11];
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
static inline unsigned int xf_blocks(uint64_t n) { return (unsigned int)((n + 255) / 256); }

void launch_unpack_scene(hipStream_t s, uint64_t n, uint32_t fields, float* pos4, float* cov3d, float* opacity, float* sh,
                         const unsigned int* orig, const float4* planes) {
    if (!n || !fields) return;
    hipLaunchKernelGGL(unpack_kernel<false>, dim3(xf_blocks(n)), dim3(256), 0, s, n, n, fields, pos4, cov3d, opacity, sh, orig,
                       (const unsigned int*)nullptr, (const unsigned int*)nullptr, planes);
}

void launch_unpack_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, uint32_t fields, float* pos4,
                           float* cov3d, float* opacity, float* sh, const unsigned int* inv, const float4* planes) {
    if (!k || !fields) return;
    hipLaunchKernelGGL(unpack_kernel<true>, dim3(xf_blocks(k)), dim3(256), 0, s, n, k, fields, pos4, cov3d, opacity, sh,
                       (const unsigned int*)nullptr, index, inv, planes);
}

static inline SplatAffine xf_affine(const float m[12]) {
    SplatAffine a;
    for (int i = 0; i < 12; ++i) a.m[i] = m[i];
    return a;
}

void launch_transform_scene(hipStream_t s, uint64_t n, const float m[12], float4* planes) {
    if (!n) return;
    hipLaunchKernelGGL(transform_kernel<false>, dim3(xf_blocks(n)), dim3(256), 0, s, n, n, xf_affine(m),
                       (const unsigned int*)nullptr, (const unsigned int*)nullptr, planes, (unsigned char*)nullptr);
}

void launch_transform_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const float m[12],
                              const unsigned int* inv, float4* planes, unsigned char* dirty) {
    if (!k) return;
    hipLaunchKernelGGL(transform_kernel<true>, dim3(xf_blocks(k)), dim3(256), 0, s, n, k, xf_affine(m), index, inv, planes, dirty);
}

void launch_rotate_sh_scene(hipStream_t s, uint64_t n, const SplatShBlocks& b, float4* planes) {
    if (!n) return;
    hipLaunchKernelGGL(rotate_sh_kernel<false>, dim3(xf_blocks(n)), dim3(256), 0, s, n, n, b, (const unsigned int*)nullptr,
                       (const unsigned int*)nullptr, planes);
}

void launch_rotate_sh_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const SplatShBlocks& b,
                              const unsigned int* inv, float4* planes) {
    if (!k) return;
    hipLaunchKernelGGL(rotate_sh_kernel<true>, dim3(xf_blocks(k)), dim3(256), 0, s, n, k, b, index, inv, planes);
}

}  // namespace splat
