// splat_neighbours.hip -- a selection by neighbourhood (splat_select_neighbours_device; gfx950): for every Gaussian of the
// resident scene, how many OTHER Gaussians of a source set have their centre within a radius of its own.
//
//   nb_block_pairs_kernel        the work bound: the ordered pairs (target block, source block) of K1 blocks whose resident
//                                bounds are within reach of each other, one workgroup per target block
//   nb_count_kernel<MASKED>      the counts: one workgroup per target block, one target slot per thread
//   nb_apply_kernel              counts -> bytes under the op, one thread per ORIGINAL index, and the count of what is selected
//
// Both predicates are splat_neighbour_math.h's, and culling by them is exact (the argument stands there): a source block is
// skipped by a workgroup whose block's bounds it cannot reach, and by a wave none of whose lanes' own centres can reach its
// bounds, and the counts are those of all pairs bit for bit.  The bounds are the resident ones, recomputed by every edit, and
// the centres the resident ones: nothing rests on the slots still being in Morton order -- a stale order costs time only.
//
// The count kernel finds its source blocks itself, 256 bounds a round, and does not read a list left by the pair kernel:
// the rescan is n_blocks box tests per workgroup (5 860 at 1.5 M Gaussians, 23 rounds) against 256 x 256 point tests for
// every block that survives, and a list would be a temporary of 4 bytes per block pair -- the very number the call bounds.
// The op is applied by a kernel of its own behind the counts, so every source byte has been read before any selection
// byte is written: d_source may be d_selection.
#include "splat_internal.h"
#include "splat_neighbour_math.h"

namespace splat {

// ---------------------------------------------------------------------------
// The work bound.  Workgroup b: target block b against every source block, thread t the blocks t, t + 256, ...; a ballot and
// a popcount per wave, the four summed in LDS, one atomic per workgroup that found any (its own block pairs with itself
// unless its bounds are NaN).  The source mask plays no part.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nb_block_pairs_kernel(unsigned int nb, const BlockBounds* __restrict__ bounds, float r2,
                                                             unsigned long long* __restrict__ pairs) {
    __shared__ unsigned int wsum[4];
    const BlockBounds tb = bounds[blockIdx.x];                 // (uniform)
    unsigned int mine = 0u;
    for (unsigned int s = threadIdx.x; s < nb; s += 256u) {
        const BlockBounds sb = bounds[s];
        mine += nb_boxes_in_reach(sb.lo, sb.hi, tb.lo, tb.hi, r2) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) mine += __shfl_xor(mine, k);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (t) atomicAdd(pairs, (unsigned long long)t);
    }
}

// ---------------------------------------------------------------------------
// The counts.  Workgroup b holds target block b, thread t its slot 256 b + t.  The source blocks are walked in rounds of
// 256: thread t tests the bounds of block base + t against the target block's, and the survivors are compacted into
// `list` (ballot ranks, in block order).  Each survivor's 256 centres are staged into LDS as float4, through two buffers --
// the loads of the next survivor are in flight while this one is counted -- with x = NaN in every slot that is no source
// (beyond n, or MASKED and source[orig[slot]] == 0): a NaN d2 fails <=, so the inner loop has no branch.  A wave skips a
// staged block that none of its unsaturated lanes' centres can reach; otherwise every lane runs over the 256 entries, all
// lanes reading the same one (LDS broadcast), 32 at a time, and the wave leaves between two runs of 32 once every lane
// has reached `cap` (count_max + 1; 0xFFFFFFFF: no bound).  In the target block itself entry threadIdx.x is the lane's own
// Gaussian: where the loop counts it (a finite centre that is a source: d2 = 0) the run that holds it takes it off again.
// counts[orig[slot]] = min(count, cap).  No atomics; 9 KB of LDS.
// ---------------------------------------------------------------------------
constexpr unsigned int NB_RUN = 32u;            // staged entries between two looks at the wave's saturation

template <bool MASKED>
static __device__ __forceinline__ float4 nb_load_source(uint64_t n, const float4* __restrict__ planes, const unsigned int* __restrict__ orig,
                                                        const unsigned char* __restrict__ source, unsigned int block) {
    const uint64_t j = (uint64_t)block * 256u + threadIdx.x;
    float4 v = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
    if (j < n) {
        v = planes[j];
        if (MASKED && source[orig[j]] == 0) v.x = __builtin_nanf("");
    }
    return v;
}

template <bool MASKED>
__global__ __launch_bounds__(256) void nb_count_kernel(uint64_t n, unsigned int nb, const float4* __restrict__ planes,
                                                       const unsigned int* __restrict__ orig, const BlockBounds* __restrict__ bounds,
                                                       const unsigned char* __restrict__ source, float r2, unsigned int cap,
                                                       unsigned int* __restrict__ counts) {
    __shared__ float4 stage[2][256];
    __shared__ unsigned int list[256];
    __shared__ unsigned int wtot[4];
    const unsigned int tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const unsigned int tblock = blockIdx.x;
    const BlockBounds tb = bounds[tblock];                     // (uniform)
    const uint64_t slot = (uint64_t)tblock * 256u + tid;
    const bool live = slot < n;
    float px = __builtin_nanf(""), py = 0.0f, pz = 0.0f;       // (a lane without a slot reaches nothing)
    if (live) { const float4 p = planes[slot]; px = p.x; py = p.y; pz = p.z; }
    unsigned int c = 0u, it = 0u;

    for (unsigned int base = 0u; base < nb; base += 256u) {    // (uniform)
        __syncthreads();                                       // (the last round's list and totals have served)
        const unsigned int s = base + tid;
        bool near = false;
        if (s < nb) { const BlockBounds sb = bounds[s]; near = nb_boxes_in_reach(sb.lo, sb.hi, tb.lo, tb.hi, r2); }
        const unsigned long long m = __ballot(near);
        const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
        if (lane == 0u) wtot[w] = (unsigned int)__popcll(m);
        __syncthreads();
        unsigned int before = 0u;
        for (unsigned int k = 0u; k < w; ++k) before += wtot[k];
        const unsigned int total = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
        if (near) list[before + rank] = s;
        __syncthreads();

        float4 next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (total) next = nb_load_source<MASKED>(n, planes, orig, source, list[0]);
        for (unsigned int e = 0u; e < total; ++e, ++it) {      // (uniform)
            const unsigned int sblock = __builtin_amdgcn_readfirstlane(list[e]);
            float4* const buf = stage[it & 1u];
            buf[tid] = next;
            __syncthreads();                                   // (the other buffer was read two syncs ago)
            if (e + 1u < total) next = nb_load_source<MASKED>(n, planes, orig, source, list[e + 1u]);
            const BlockBounds sb = bounds[sblock];             // (uniform)
            const bool want = c < cap && nb_point_in_reach(sb.lo, sb.hi, px, py, pz, r2);
            if (__ballot(want) == 0ull) continue;              // (wave-uniform; no barrier below)
            // the lane's own Gaussian, staged with its own block: counted by the run that holds entry tid, taken off again
            const bool own = sblock == tblock && nb_within_reach(px, py, pz, buf[tid].x, buf[tid].y, buf[tid].z, r2);
#pragma unroll 1
            for (unsigned int k0 = 0u; k0 < 256u; k0 += NB_RUN) {
                unsigned int hits = 0u;
#pragma unroll 8
                for (unsigned int k = k0; k < k0 + NB_RUN; ++k) {
                    const float4 q = buf[k];                   // (every lane the same entry)
                    hits += nb_within_reach(px, py, pz, q.x, q.y, q.z, r2) ? 1u : 0u;
                }
                hits -= (own && tid - k0 < NB_RUN) ? 1u : 0u;
                c = min(c + hits, cap);                        // (no wrap: c + hits is at most the full count, below n < 2^32)
                if (__ballot(c < cap) == 0ull) break;
            }
        }
    }
    if (live) counts[orig[slot]] = c;
}

// ---------------------------------------------------------------------------
// Counts -> bytes.  Thread i judges Gaussian i (ORIGINAL index): it passes when count_min <= counts[i] <= count_max -- a count
// saturated at count_max + 1 fails as the full one would -- and its byte is combined as select_kernel combines it.
// selection == nullptr (a counts-only call): nothing is written and *count += the Gaussians that pass.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nb_apply_kernel(uint64_t n, const unsigned int* __restrict__ counts, unsigned int count_min,
                                                       unsigned int count_max, uint32_t op, unsigned char* selection,
                                                       unsigned int* __restrict__ count) {
    __shared__ unsigned int wsel[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool sel = false;
    if (i < n) {
        const unsigned int c = counts[i];
        const bool pass = count_min <= c && c <= count_max;
        if (!selection) sel = pass;
        else {
            unsigned char* const b = selection + i;
            if (op == SPLAT_SEL_OP_SET) { sel = pass; *b = (unsigned char)(pass ? 1 : 0); }
            else {
                const bool old = *b != 0;
                if (op == SPLAT_SEL_OP_ADD) { sel = old || pass; if (pass) *b = (unsigned char)1; }
                else if (op == SPLAT_SEL_OP_SUBTRACT) { sel = old && !pass; if (pass) *b = (unsigned char)0; }
                else { sel = old && pass; *b = (unsigned char)(sel ? 1 : 0); }
            }
        }
    }
    const unsigned long long m = __ballot(sel);
    if ((threadIdx.x & 63u) == 0u) wsel[threadIdx.x >> 6] = (unsigned int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = (wsel[0] + wsel[1]) + (wsel[2] + wsel[3]);
        if (t) atomicAdd(count, t);
    }
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
void launch_neighbour_block_pairs(hipStream_t s, uint64_t n, const BlockBounds* bounds, float r2, unsigned long long* pairs) {
    if (!n) return;
    const unsigned int nb = (unsigned int)((n + 255) / 256);
    hipLaunchKernelGGL(nb_block_pairs_kernel, dim3(nb), dim3(256), 0, s, nb, bounds, r2, pairs);
}

void launch_neighbour_counts(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const BlockBounds* bounds,
                             const unsigned char* source, float r2, unsigned int cap, unsigned int* counts) {
    if (!n) return;
    const unsigned int nb = (unsigned int)((n + 255) / 256);
    if (source) hipLaunchKernelGGL(nb_count_kernel<true>, dim3(nb), dim3(256), 0, s, n, nb, planes, orig, bounds, source, r2, cap, counts);
    else hipLaunchKernelGGL(nb_count_kernel<false>, dim3(nb), dim3(256), 0, s, n, nb, planes, orig, bounds, source, r2, cap, counts);
}

void launch_neighbour_apply(hipStream_t s, uint64_t n, const unsigned int* counts, unsigned int count_min, unsigned int count_max,
                            uint32_t op, unsigned char* selection, unsigned int* count) {
    if (!n) return;
    hipLaunchKernelGGL(nb_apply_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, n, counts, count_min, count_max, op,
                       selection, count);
}

}  // namespace splat
