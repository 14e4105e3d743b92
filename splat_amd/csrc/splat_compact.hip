// splat_compact.hip -- Gaussians taken out of the resident scene, the survivors compacted (splat_remove_gaussians_device; gfx950).
//
//   index_map_kernel         map[i] = the new index of Gaussian i -- its rank among the survivors, in original index order -- or
//                            REMOVED_INDEX; walks the caller's mask in the spans of mask_count_kernel, behind its scanned counts
//   slot_keep_count_kernel   how many slots of a K1 block hold a survivor (map[orig[slot]] is an index), per block
//   compact_scene_kernel     the survivors' sixteen planes and their new indices gathered to consecutive slots, in slot order
//
// The scene's order is kept: slot order among the survivors is what it was, and a subsequence of a Morton-ordered scene is
// Morton-ordered, so nothing is sorted.  Two prefix sums (mask_scan_kernel of splat_select.hip: over the mask's spans, over the
// blocks' kept slots) and one streaming gather: 256 B read and 256 B written per survivor.  Every destination is a rank --
// scanned counts, ballots, mbcnt -- never the arrival order of an atomic; no kernel waits on another workgroup.  The bounds
// of the new blocks are plane_bounds_kernel's (splat_update.hip), run behind the gather.
#include "splat_internal.h"
#include "splat_mask.h"

namespace splat {

// offsets: the scanned counts of the mask's spans (selected bytes in front of each).  With s the selected bytes in front
// of byte i: under SPLAT_REMOVE_UNSELECTED the selected stay and i's new index is s, under SPLAT_REMOVE_SELECTED the others
// stay and it is i - s.  Every map[i], 0 <= i < n, is written, by the one lane that holds byte i's chunk.
__global__ __launch_bounds__(256) void index_map_kernel(uint64_t n, const unsigned char* __restrict__ mask, unsigned int head,
                                                        const unsigned int* __restrict__ offsets, uint32_t mode,
                                                        unsigned int* __restrict__ map) {
    __shared__ unsigned int wtot[4];
    int64_t first;
    const unsigned int bits = chunk_bits(mask, n, head, (uint64_t)blockIdx.x * 256u + threadIdx.x, &first);
    unsigned int tot;
    const unsigned int rank = wave_rank(bits, &tot);
    const unsigned int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wtot[w] = tot;
    __syncthreads();
    unsigned int s = offsets[blockIdx.x] + rank;
    for (unsigned int k = 0; k < w; ++k) s += wtot[k];
    const bool keep_selected = mode == SPLAT_REMOVE_UNSELECTED;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t i = first + k;
        const bool sel = (bits >> k) & 1u;
        if (i >= 0 && i < (int64_t)n) map[i] = (sel != keep_selected) ? REMOVED_INDEX : (keep_selected ? s : (unsigned int)i - s);
        s += sel ? 1u : 0u;
    }
}

// thread t of workgroup b holds slot 256 b + t; *kept: whether it holds a survivor.  Returns map[orig[slot]].
static __device__ __forceinline__ unsigned int slot_new_index(uint64_t n, const unsigned int* __restrict__ orig,
                                                              const unsigned int* __restrict__ map, uint64_t j, bool* kept) {
    const unsigned int m = j < n ? map[orig[j]] : REMOVED_INDEX;
    *kept = m != REMOVED_INDEX;
    return m;
}

// a ballot and a popcount per wave, the four summed in LDS: one count per block
__global__ __launch_bounds__(256) void slot_keep_count_kernel(uint64_t n, const unsigned int* __restrict__ orig,
                                                              const unsigned int* __restrict__ map, unsigned int* __restrict__ counts) {
    __shared__ unsigned int wtot[4];
    bool kept;
    (void)slot_new_index(n, orig, map, (uint64_t)blockIdx.x * 256u + threadIdx.x, &kept);
    const unsigned long long b = __ballot(kept);
    if ((threadIdx.x & 63u) == 0u) wtot[threadIdx.x >> 6] = (unsigned int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// offsets: the scanned counts of the kernel above.  A kept lane's destination is offsets[block] + the kept lanes of the waves
// below its own + the kept lanes below it in its wave (mbcnt): slot order is kept, and the kept lanes of a wave write
// consecutive slots of every plane.  All sixteen planes of the old slot are loaded before the first is stored: sixteen
// independent 16-byte loads in flight per lane, no load behind a store.  n2: the survivors -- no destination is at or beyond
// it when map and offsets are what the kernels above made of one mask; a lane that would be is dropped, not stored.
__global__ __launch_bounds__(256) void compact_scene_kernel(uint64_t n, uint64_t n2, const float4* __restrict__ planes,
                                                            const unsigned int* __restrict__ orig, const unsigned int* __restrict__ map,
                                                            const unsigned int* __restrict__ offsets, float4* __restrict__ planes2,
                                                            unsigned int* __restrict__ orig2) {
    __shared__ unsigned int wtot[4];
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool kept;
    const unsigned int m = slot_new_index(n, orig, map, j, &kept);
    const unsigned long long b = __ballot(kept);
    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)b, 0u));
    const unsigned int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wtot[w] = (unsigned int)__popcll(b);
    __syncthreads();
    uint64_t d = (uint64_t)offsets[blockIdx.x] + rank;
    for (unsigned int k = 0; k < w; ++k) d += wtot[k];
    if (!kept || d >= n2) return;
    float4 v[SCENE_PLANES];
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p) v[p] = planes[(uint64_t)p * n + j];
#pragma unroll
    for (int p = 0; p < SCENE_PLANES; ++p) planes2[(uint64_t)p * n2 + d] = v[p];
    orig2[d] = m;
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
void launch_index_map(hipStream_t s, uint64_t n, const unsigned char* mask, const unsigned int* offsets, uint32_t mode,
                      unsigned int* map) {
    if (!n) return;
    const unsigned int head = (unsigned int)((uintptr_t)mask & 15u);
    const unsigned int g = (unsigned int)selection_groups(mask, n);
    hipLaunchKernelGGL(index_map_kernel, dim3(g), dim3(256), 0, s, n, mask, head, offsets, mode, map);
}

void launch_compact_scene(hipStream_t s, uint64_t n, uint64_t n2, const float4* planes, const unsigned int* orig,
                          const unsigned int* map, unsigned int* block_counts, float4* planes2, unsigned int* orig2) {
    if (!n) return;
    const unsigned int nb = (unsigned int)((n + 255) / 256);
    hipLaunchKernelGGL(slot_keep_count_kernel, dim3(nb), dim3(256), 0, s, n, orig, map, block_counts);
    launch_count_scan(s, nb, block_counts);
    hipLaunchKernelGGL(compact_scene_kernel, dim3(nb), dim3(256), 0, s, n, n2, planes, orig, map, (const unsigned int*)block_counts,
                       planes2, orig2);
}

}  // namespace splat
