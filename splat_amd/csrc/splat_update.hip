// splat_update.hip -- a resident scene edited in place (splat_update_scene_device, splat_update_gaussians_device; gfx950).
//
//   inverse_order_kernel     inv[orig[j]] = j: the slot of every original index (built once per scene, for the indexed form)
//   index_check_kernel       how many of the caller's indices are >= n (read back before anything is written)
//   repack_kernel<INDEXED>   the named fields' float slots of the planes rewritten, the others kept
//   plane_bounds_kernel      the bounds of a K1 block from the planes: block_bounds_kernel's reduction, other loads
//
// The order of the scene (orig[]) stays as the last upload left it.  A frame does not depend on it -- depth ties are settled
// through orig[] and the bounds only cull -- so the frames that follow are those of a fresh upload of the edited arrays.
// The bounds are block_bounds' of splat_scene.hip, bit for bit: the planes hold the very floats the caller's buffers held.
#include "splat_internal.h"

namespace splat {

// (as in splat_kernels.hip: the EARLIER of two equal values stays -- +0 and -0 differ in the bounds' bits)
static __device__ __forceinline__ bool upd_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }
static __device__ __forceinline__ float upd_min_keep_first(float a, float b) { return (b < a) ? b : a; }
static __device__ __forceinline__ float upd_max_keep_first(float a, float b) { return (a < b) ? b : a; }

__global__ __launch_bounds__(256) void inverse_order_kernel(uint64_t n, const unsigned int* __restrict__ orig, unsigned int* __restrict__ inv) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j < n) inv[orig[j]] = (unsigned int)j;                 // (orig is a permutation of 0 .. n-1)
}

// *bad += the indices of index[0..k) that name no Gaussian: one integer atomic per wave that found any
__global__ __launch_bounds__(256) void index_check_kernel(uint64_t k, uint64_t n, const unsigned int* __restrict__ index, unsigned int* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool out = t < k && (uint64_t)index[t] >= n;
    const unsigned long long m = __ballot(out);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(bad, (unsigned int)__popcll(m));
}

// ---------------------------------------------------------------------------
// Masked repack.  Float slots of a Gaussian as pack_scene_kernel lays them out: 0-2 xyz, 3 opacity, 4-12 cov3d, 13-60 sh,
// 61-63 zero; plane p holds slots 4p .. 4p+3.  Two planes are shared between fields -- plane 0 (x y z | opacity) and plane 3
// (cov[8] | sh0 sh1 sh2): unless both of a shared plane's fields are named, its resident float4 is read, the named part
// replaced, and the whole written back.  A slot belongs to one thread (the indices are distinct), so nothing races.
// INDEXED = false: thread j rewrites slot j from row orig[j] of the caller's buffers (rows == n).
// INDEXED = true:  thread t rewrites slot inv[index[t]] from row t of the COMPACT buffers (rows == k), and marks the slot's
// block dirty when the bounds will be recomputed (dirty != nullptr): a plain byte store of 1, the same value from every
// thread that stores it.
// (amdgpu_waves_per_eu(8): the 48 sh loads would otherwise all be in flight at once, at 66-68 VGPRs; eight waves a SIMD hold
// the kernel to 64 and hide the same latency)
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8)))
void repack_kernel(uint64_t n, uint64_t rows, uint32_t fields, const float* __restrict__ pos4,
                   const float* __restrict__ cov3d, const float* __restrict__ opacity, const float* __restrict__ sh,
                   const unsigned int* __restrict__ orig, const unsigned int* __restrict__ index,
                   const unsigned int* __restrict__ inv, float4* __restrict__ planes, unsigned char* __restrict__ dirty) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= rows) return;
    uint64_t j, r;                                             // the slot written, the row read
    if (INDEXED) { r = t; j = inv[index[t]]; } else { j = t; r = orig[t]; }
    const bool f_pos = fields & SPLAT_FIELD_POS, f_cov = fields & SPLAT_FIELD_COV3D, f_op = fields & SPLAT_FIELD_OPACITY,
               f_sh = fields & SPLAT_FIELD_SH;
    if (f_pos || f_op) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!(f_pos && f_op)) v = planes[j];
        if (f_pos) { v.x = pos4[4 * r]; v.y = pos4[4 * r + 1]; v.z = pos4[4 * r + 2]; }
        if (f_op) v.w = opacity[r];
        planes[j] = v;
    }
    if (f_cov) {
        const float* c = cov3d + 9 * r;
        planes[n + j] = make_float4(c[0], c[1], c[2], c[3]);
        planes[2 * n + j] = make_float4(c[4], c[5], c[6], c[7]);
    }
    if (f_cov || f_sh) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!(f_cov && f_sh)) v = planes[3 * n + j];
        if (f_cov) v.x = cov3d[9 * r + 8];
        if (f_sh) { v.y = sh[48 * r]; v.z = sh[48 * r + 1]; v.w = sh[48 * r + 2]; }
        planes[3 * n + j] = v;
    }
    if (f_sh) {
        const float* q = sh + 48 * r + 3;                      // plane p, 4 <= p <= 14: sh[4p - 13 .. 4p - 10]
#pragma unroll
        for (int p = 4; p < 15; ++p, q += 4) planes[(uint64_t)p * n + j] = make_float4(q[0], q[1], q[2], q[3]);
        planes[15 * n + j] = make_float4(q[0], 0.0f, 0.0f, 0.0f);      // sh[47] and the three slots nothing reads
    }
    if (INDEXED && dirty) dirty[j >> 8] = (unsigned char)1;
}

// ---------------------------------------------------------------------------
// Bounds of K1 block blockIdx.x from the planes: thread t holds slot 256 b + t.  block_bounds_kernel of splat_kernels.hip
// with the centre read from plane 0 and the nine covariance floats from planes 1, 2 and 3.x, in their order.
// dirty != nullptr (the indexed form, launched over all blocks): a workgroup whose byte is 0 leaves at once; the one that
// recomputes its block clears the byte it consumed.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void plane_bounds_kernel(uint64_t n, const float4* __restrict__ planes, unsigned char* dirty,
                                                           BlockBounds* __restrict__ out) {
    __shared__ float red[4][7];
    if (dirty && dirty[blockIdx.x] == 0) return;               // (uniform)
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, fmax = 0.0f;
    if (j < n) {
        const float4 p = planes[j];
        if (upd_finite(p.x) && upd_finite(p.y) && upd_finite(p.z)) {
            lo[0] = hi[0] = p.x; lo[1] = hi[1] = p.y; lo[2] = hi[2] = p.z;
            const float4 c0 = planes[n + j], c1 = planes[2 * n + j];
            const float c8 = planes[3 * n + j].x;
            const float cov[9] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c8};
            double f2 = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) { const double v = (double)cov[e]; f2 += v * v; }
            float f = (float)sqrt(f2) * 1.0001f;
            if (!(f >= 0.0f)) f = INFINITY;                    // NaN: unbounded extent
            fmax = f;
        }
    }
    // lane l ends up with the lanes l .. 63 in order (strides 1, 2, 4, ...: neighbouring runs joined, the earlier one on the left)
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = upd_min_keep_first(lo[a], __shfl_down(lo[a], k));
            hi[a] = upd_max_keep_first(hi[a], __shfl_down(hi[a], k));
        }
        fmax = upd_max_keep_first(fmax, __shfl_down(fmax, k));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[w][a] = lo[a]; red[w][3 + a] = hi[a]; }
        red[w][6] = fmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        BlockBounds bb;
        for (int a = 0; a < 3; ++a) {
            float l = red[0][a], h = red[0][3 + a];
            for (int k = 1; k < 4; ++k) { l = upd_min_keep_first(l, red[k][a]); h = upd_max_keep_first(h, red[k][3 + a]); }
            bb.lo[a] = l; bb.hi[a] = h;
        }
        float f = red[0][6];
        for (int k = 1; k < 4; ++k) f = upd_max_keep_first(f, red[k][6]);
        bb.fmax = f; bb.pad = 0.0f;
        if (!(bb.lo[0] <= bb.hi[0]))                            // no finite centre at all: NaN bounds answer "maybe"
            for (int a = 0; a < 3; ++a) { bb.lo[a] = NAN; bb.hi[a] = NAN; }
        out[blockIdx.x] = bb;
        if (dirty) dirty[blockIdx.x] = (unsigned char)0;
    }
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
static inline unsigned int upd_blocks(uint64_t n) { return (unsigned int)((n + 255) / 256); }

void launch_inverse_order(hipStream_t s, uint64_t n, const unsigned int* orig, unsigned int* inv) {
    if (!n) return;
    hipLaunchKernelGGL(inverse_order_kernel, dim3(upd_blocks(n)), dim3(256), 0, s, n, orig, inv);
}

void launch_index_check(hipStream_t s, uint64_t k, uint64_t n, const unsigned int* index, unsigned int* bad) {
    if (!k) return;
    hipLaunchKernelGGL(index_check_kernel, dim3(upd_blocks(k)), dim3(256), 0, s, k, n, index, bad);
}

void launch_repack_scene(hipStream_t s, uint64_t n, uint32_t fields, const float* pos4, const float* cov3d, const float* opacity,
                         const float* sh, const unsigned int* orig, float4* planes) {
    if (!n || !fields) return;
    hipLaunchKernelGGL(repack_kernel<false>, dim3(upd_blocks(n)), dim3(256), 0, s, n, n, fields, pos4, cov3d, opacity, sh, orig,
                       (const unsigned int*)nullptr, (const unsigned int*)nullptr, planes, (unsigned char*)nullptr);
}

void launch_repack_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, uint32_t fields, const float* pos4,
                           const float* cov3d, const float* opacity, const float* sh, const unsigned int* inv, float4* planes,
                           unsigned char* dirty) {
    if (!k || !fields) return;
    hipLaunchKernelGGL(repack_kernel<true>, dim3(upd_blocks(k)), dim3(256), 0, s, n, k, fields, pos4, cov3d, opacity, sh,
                       (const unsigned int*)nullptr, index, inv, planes, dirty);
}

void launch_plane_bounds(hipStream_t s, uint64_t n, const float4* planes, unsigned char* dirty, BlockBounds* bounds) {
    if (!n) return;
    hipLaunchKernelGGL(plane_bounds_kernel, dim3(upd_blocks(n)), dim3(256), 0, s, n, planes, dirty, bounds);
}

}  // namespace splat
