// splat_select.hip -- a selection made from the resident scene, and its indices (splat_select_device,
// splat_selection_indices_device; gfx950).
//
//   select_kernel<LEVEL, CORRECTED>   one thread per stored slot: the query's tests on the resident values, combined with the
//                                     caller's byte at selection[orig[slot]], and the count of what is selected afterwards
//   mask_count_kernel                 how many bytes of a span of the mask are nonzero, per workgroup
//   mask_scan_kernel                  one workgroup: the exclusive prefix sums of those counts, 256 of them a round
//   mask_scatter_kernel               the positions of a span's nonzero bytes, written behind those of the spans before it
//
// The SCREEN test is the geometry half of K1 (preprocess_kernel of splat_kernels.hip) restated (splat_project.h): the same f32 operations in
// the same order (project_cov3d_to_screen, the conic, the half extents, NDC to pixels, visibility, covered_interval), built
// with the same flags -- no contraction, correctly rounded division and square root -- so the same bits: a Gaussian is
// selected by the very centre and covered range the frame draws it with (tests/test_gpu_select.py holds it to the oracle).
// The compaction never waits on another workgroup: three launches, each reading what the one before it wrote.
#include "splat_internal.h"
#include "splat_mask.h"
#include "splat_project.h"

namespace splat {

// ---------------------------------------------------------------------------
// The predicate.  LEVEL: what the named tests need of the camera -- 0: nothing (VOLUME, OPACITY: plane 0 alone is read),
// 1: view-space z (DEPTH: one row of the view matrix), 2: the projected Gaussian (SCREEN: planes 0-3).  No SH is loaded.
// The byte of a Gaussian belongs to the one thread that holds its slot (orig is a permutation): nothing races.
// ---------------------------------------------------------------------------
template <int LEVEL, bool CORRECTED>
__global__ __launch_bounds__(256) void select_kernel(uint64_t n, const float4* __restrict__ planes, const unsigned int* __restrict__ orig,
                                                     splat_select_query q, SelectView fc, const unsigned char* __restrict__ pixel_mask,
                                                     uint32_t op, unsigned char* selection, unsigned int* __restrict__ count) {
    __shared__ unsigned int wsel[4];
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool sel = false;
    if (j < n) {
        const float4 p0 = planes[j];                           // x y z | opacity
        bool pass = true;
        if (q.tests & SPLAT_SEL_VOLUME) {
            const float* m = q.world_to_unit;
            float u[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) u[k] = ((m[4 * k] * p0.x + m[4 * k + 1] * p0.y) + m[4 * k + 2] * p0.z) + m[4 * k + 3];
            if (q.volume_shape == 0u) pass = (fabsf(u[0]) <= 1.0f) && (fabsf(u[1]) <= 1.0f) && (fabsf(u[2]) <= 1.0f);
            else pass = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) <= 1.0f;
        }
        if (q.tests & SPLAT_SEL_OPACITY) pass = pass && (q.opacity_min <= p0.w) && (p0.w <= q.opacity_max);
        if (LEVEL >= 1 && (q.tests & SPLAT_SEL_DEPTH)) {
            const float z = sel_mat4_row(fc.view, 2, p0.x, p0.y, p0.z, 1.0f);
            pass = pass && (q.depth_min <= z) && (z <= q.depth_max);
        }
        if (LEVEL >= 2) {                                      // (launched only with SCREEN named)
            const float4 c0 = planes[n + j], c1 = planes[2 * n + j];
            const float c8 = planes[3 * n + j].x;
            const float c9[9] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c8};
            float cx, cy; int r[4] = {1, 0, 1, 0};
            bool hit = sel_project<CORRECTED>(fc, p0.x, p0.y, p0.z, c9, &cx, &cy, r) && q.x0 <= q.x1 && q.y0 <= q.y1;
            if (hit) {
                if (q.screen_rule == 0u) {
                    hit = ((float)q.x0 <= cx) && (cx < (float)(q.x1 + 1)) && ((float)q.y0 <= cy) && (cy < (float)(q.y1 + 1));
                    // (inside the clamped rectangle: 0 <= (int)cx < W and 0 <= (int)cy < H)
                    if (hit && pixel_mask) hit = pixel_mask[(size_t)(int)cy * (size_t)fc.W + (size_t)(int)cx] != 0;
                } else {
                    hit = r[0] <= q.x1 && r[1] >= q.x0 && r[2] <= q.y1 && r[3] >= q.y0;
                }
            }
            pass = pass && hit;
        }
        unsigned char* const b = selection + orig[j];
        if (op == SPLAT_SEL_OP_SET) { sel = pass; *b = (unsigned char)(pass ? 1 : 0); }
        else {
            const bool old = *b != 0;
            if (op == SPLAT_SEL_OP_ADD) { sel = old || pass; if (pass) *b = (unsigned char)1; }
            else if (op == SPLAT_SEL_OP_SUBTRACT) { sel = old && !pass; if (pass) *b = (unsigned char)0; }
            else { sel = old && pass; *b = (unsigned char)(sel ? 1 : 0); }
        }
    }
    // the count: a ballot and a popcount per wave, the four summed in LDS, one atomic per workgroup that selected any
    const unsigned long long m = __ballot(sel);
    if ((threadIdx.x & 63u) == 0u) wsel[threadIdx.x >> 6] = (unsigned int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = (wsel[0] + wsel[1]) + (wsel[2] + wsel[3]);
        if (t) atomicAdd(count, t);
    }
}

// ---------------------------------------------------------------------------
// Compaction.  How the mask is read in chunks at any byte address (chunk_bits) and how a lane's selected bytes rank in its
// wave (wave_rank): splat_mask.h, shared with the removal's index map.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_count_kernel(uint64_t n, const unsigned char* __restrict__ mask, unsigned int head,
                                                         unsigned int* __restrict__ counts) {
    __shared__ unsigned int wtot[4];
    int64_t first;
    const unsigned int bits = chunk_bits(mask, n, head, (uint64_t)blockIdx.x * 256u + threadIdx.x, &first);
    unsigned int tot;
    (void)wave_rank(bits, &tot);
    if ((threadIdx.x & 63u) == 0u) wtot[threadIdx.x >> 6] = tot;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// counts[0..g) -> their exclusive prefix sums, counts[g] = the total.  ONE workgroup, SELECT_SCAN_ROUND counts a round with
// the sum so far carried from round to round (every thread carries the same one): as many rounds as it takes.
__global__ __launch_bounds__(256) void mask_scan_kernel(unsigned int g, unsigned int* __restrict__ counts) {
    static_assert(SELECT_SCAN_ROUND == 256u, "one count per thread and round");
    __shared__ unsigned int wsum[4];
    const unsigned int lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned int carry = 0u;
    for (unsigned int base = 0u; base < g; base += SELECT_SCAN_ROUND) {            // (uniform)
        const unsigned int i = base + threadIdx.x;
        const unsigned int v = i < g ? counts[i] : 0u;
        unsigned int inc = v;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const unsigned int below = __shfl_up(inc, k);
            if (lane >= (unsigned int)k) inc += below;
        }
        if (lane == 63u) wsum[w] = inc;
        __syncthreads();
        unsigned int before = 0u;
        for (unsigned int k = 0; k < w; ++k) before += wsum[k];
        const unsigned int round = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (i < g) counts[i] = carry + before + (inc - v);
        carry += round;
        __syncthreads();                                       // (wsum is written again by the next round)
    }
    if (threadIdx.x == 0) counts[g] = carry;
}

// offsets: the scanned counts.  A lane's selected bytes land at offsets[workgroup] + those of the waves before its own +
// its rank in the wave, in index order: the output is ascending.  Entries beyond `capacity` are not written.
__global__ __launch_bounds__(256) void mask_scatter_kernel(uint64_t n, const unsigned char* __restrict__ mask, unsigned int head,
                                                           const unsigned int* __restrict__ offsets, unsigned int* __restrict__ out,
                                                           uint64_t capacity) {
    __shared__ unsigned int wtot[4];
    int64_t first;
    unsigned int bits = chunk_bits(mask, n, head, (uint64_t)blockIdx.x * 256u + threadIdx.x, &first);
    unsigned int tot;
    const unsigned int rank = wave_rank(bits, &tot);
    const unsigned int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wtot[w] = tot;
    __syncthreads();
    uint64_t pos = (uint64_t)offsets[blockIdx.x] + rank;
    for (unsigned int k = 0; k < w; ++k) pos += wtot[k];
    while (bits != 0u && pos < capacity) {
        const int k = __builtin_ctz(bits);
        bits &= bits - 1u;
        out[pos++] = (unsigned int)(first + k);
    }
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
void launch_select_query(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const splat_select_query& q,
                         const SelectView& v, const unsigned char* pixel_mask, uint32_t op, unsigned char* selection,
                         unsigned int* count) {
    if (!n) return;
    const dim3 grid((unsigned int)((n + 255) / 256)), block(256);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, n, planes, orig, q, v, pixel_mask, op, selection, count); };
    if (q.tests & SPLAT_SEL_SCREEN) { if (v.corrected) go(select_kernel<2, true>); else go(select_kernel<2, false>); }
    else if (q.tests & SPLAT_SEL_DEPTH) go(select_kernel<1, false>);
    else go(select_kernel<0, false>);
}

void launch_selection_indices(hipStream_t s, uint64_t n, const unsigned char* mask, unsigned int* out, uint64_t capacity,
                              unsigned int* counts) {
    if (!n) return;
    static_assert(SELECT_SPAN == 256u * 16u, "a workgroup's span is one 16-byte chunk per thread");
    const unsigned int head = (unsigned int)((uintptr_t)mask & 15u);
    const unsigned int g = (unsigned int)selection_groups(mask, n);                // (n < 2^32: at most 2^20 + 1)
    hipLaunchKernelGGL(mask_count_kernel, dim3(g), dim3(256), 0, s, n, mask, head, counts);
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(256), 0, s, g, counts);
    if (capacity && out) hipLaunchKernelGGL(mask_scatter_kernel, dim3(g), dim3(256), 0, s, n, mask, head, (const unsigned int*)counts, out, capacity);
}

void launch_count_scan(hipStream_t s, unsigned int g, unsigned int* counts) {
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(256), 0, s, g, counts);
}

}  // namespace splat
