// splat_append.hip -- Gaussians added to the resident scene, and its slots put back in order (splat_append_gaussians_device,
// splat_reorder_scene_device; gfx950).
//
//   grow_scene_kernel      the sixteen planes and the indices of the n resident slots copied from stride n to stride n2 = n + m
//   pack_append_kernel     the m new rows packed as pack_scene_kernel (splat_kernels.hip) packs them, into the slots n .. n2-1
//                          of the same arrays, in the order launch_scene_order gave the new rows alone; their indices are n ..
//   order_moved_kernel     how many slots of a new order hold another Gaussian than they do now
//   permute_scene_kernel   new slot j filled from the old slot of the Gaussian the new order puts there
//
// An append sorts nothing but what it adds: the resident slots keep their place and the blocks wholly below slot n their
// bounds; the others get plane_bounds_kernel's (splat_update.hip).  A reorder is the sort of an upload run over the resident
// positions, and one gather: 256 B read and 256 B written per Gaussian.  Every destination is a slot number known before
// the kernel runs; no kernel waits on another workgroup.
#include "splat_internal.h"

namespace splat {

// One slot per lane.  All sixteen planes of the slot are loaded before the first is stored, as compact_scene_kernel does:
// sixteen independent 16-byte loads per lane, none of which waits for a store.
__global__ __launch_bounds__(256) void grow_scene_kernel(uint64_t n, uint64_t n2, const float4* __restrict__ planes,
                                                         const unsigned int* __restrict__ orig, float4* __restrict__ planes2,
                                                         unsigned int* __restrict__ orig2) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    float4 v[SCENE_PLANES];
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p) v[p] = planes[(uint64_t)p * n + j];
    const unsigned int i = orig[j];
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p) planes2[(uint64_t)p * n2 + j] = v[p];
    orig2[j] = i;
}

// pack_scene_kernel's packing for a destination of stride n2, slot base n and index base n.  Float slots: 0-2 xyz, 3 opacity,
// 4-12 cov3d, 13-60 sh, 61-63 zero.  tail = orig2 + n: on entry tail[j] is the row that goes to slot n + j (the order of the
// new rows alone), on exit the index that row has in the scene.  Each lane reads and writes its own word of it.
__global__ __launch_bounds__(256) void pack_append_kernel(uint64_t n, uint64_t n2, uint64_t m, const float* __restrict__ pos4,
                                                          const float* __restrict__ cov3d, const float* __restrict__ opacity,
                                                          const float* __restrict__ sh, unsigned int* tail,
                                                          float4* __restrict__ planes2) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    const uint64_t i = tail[j];
    if (i >= m) return;                        // (an order of m rows names no other)
    float F[64];
    F[0] = pos4[4 * i + 0]; F[1] = pos4[4 * i + 1]; F[2] = pos4[4 * i + 2]; F[3] = opacity[i];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[4 + k] = cov3d[9 * i + k];
#pragma unroll
    for (int k = 0; k < 48; ++k) F[13 + k] = sh[48 * i + k];
    F[61] = F[62] = F[63] = 0.0f;
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p)
        planes2[(uint64_t)p * n2 + n + j] = make_float4(F[4 * p], F[4 * p + 1], F[4 * p + 2], F[4 * p + 3]);
    tail[j] = (unsigned int)(n + i);
}

// a ballot and a popcount per wave, one 64-bit add per wave: the sum does not depend on the order of arrival
__global__ __launch_bounds__(256) void order_moved_kernel(uint64_t n, const unsigned int* __restrict__ orig,
                                                          const unsigned int* __restrict__ orig2, unsigned long long* __restrict__ moved) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool differs = j < n && orig[j] != orig2[j];
    const unsigned long long b = __ballot(differs);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(moved, (unsigned long long)__popcll(b));
}

// New slot j holds Gaussian orig2[j], which lies in old slot inv[orig2[j]]: sixteen gathered 16-byte loads, all issued before
// the first store; the stores of a wave are consecutive in every plane.  A slot number at or beyond n cannot come out of an
// order and its inverse over the same n Gaussians; a lane that had one would be dropped, not loaded.
__global__ __launch_bounds__(256) void permute_scene_kernel(uint64_t n, const float4* __restrict__ planes,
                                                            const unsigned int* __restrict__ inv, const unsigned int* __restrict__ orig2,
                                                            float4* __restrict__ planes2) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint64_t i = orig2[j];
    if (i >= n) return;
    const uint64_t s = inv[i];
    if (s >= n) return;
    float4 v[SCENE_PLANES];
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p) v[p] = planes[(uint64_t)p * n + s];
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p) planes2[(uint64_t)p * n + j] = v[p];
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
static inline unsigned int app_blocks(uint64_t n) { return (unsigned int)((n + 255) / 256); }

void launch_grow_scene(hipStream_t s, uint64_t n, uint64_t n2, const float4* planes, const unsigned int* orig, float4* planes2,
                       unsigned int* orig2) {
    if (!n) return;
    hipLaunchKernelGGL(grow_scene_kernel, dim3(app_blocks(n)), dim3(256), 0, s, n, n2, planes, orig, planes2, orig2);
}

void launch_pack_append(hipStream_t s, uint64_t n, uint64_t m, const float* pos4, const float* cov3d, const float* opacity,
                        const float* sh, float4* planes2, unsigned int* orig2) {
    if (!m) return;
    hipLaunchKernelGGL(pack_append_kernel, dim3(app_blocks(m)), dim3(256), 0, s, n, n + m, m, pos4, cov3d, opacity, sh, orig2 + n, planes2);
}

void launch_order_moved(hipStream_t s, uint64_t n, const unsigned int* orig, const unsigned int* orig2, unsigned long long* moved) {
    if (!n) return;
    hipLaunchKernelGGL(order_moved_kernel, dim3(app_blocks(n)), dim3(256), 0, s, n, orig, orig2, moved);
}

void launch_permute_scene(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* inv, const unsigned int* orig2,
                          float4* planes2) {
    if (!n) return;
    hipLaunchKernelGGL(permute_scene_kernel, dim3(app_blocks(n)), dim3(256), 0, s, n, planes, inv, orig2, planes2);
}

}  // namespace splat
