// splat_pick.hip -- what a pixel is made of, read from the resident scene (splat_pick_device; gfx950): the Gaussians whose
// fragment the reference accepts at up to 256 query pixels, nearest first, with the front one, the surface and the layers.
//
//   pick_hits_kernel<CORRECTED>   one thread per stored slot: the Gaussian projected once (splat_project.h: K1's geometry, the
//                                 selection's), its fragment evaluated at every query pixel inside its covered range
//                                 (splat_pick_math.h: the reference's fragment() with glibc's expf), and every hit counted,
//                                 offered as the pixel's front and appended to the pixel's list
//   pick_resolve_kernel           one workgroup per query pixel: the list sorted in LDS, nearest first, the coverage chain
//                                 walked by one thread, the result and the layers written
//   pick_front_kernel<CORRECTED>  one thread per stored slot, for the pixels with more hits than their list holds: the front
//                                 Gaussian found in the order and projected again for its alpha (it leaves at once otherwise)
//
// A stand-alone query: it reads the planes and the order of the scene and nothing a frame makes -- no record, no tile list,
// no compositor state -- and it is built with K1's flags (no contraction, correctly rounded division and square root), so a
// hit has the very centre, range, conic and depth the frame draws it with (tests/test_gpu_pick.py holds every field of every
// result to the oracle, bit for bit).
#include "splat_internal.h"
#include "splat_pick_math.h"
#include "splat_project.h"

namespace splat {

static_assert(PICK_MAX_PIXELS == SPLAT_PICK_MAX_PIXELS && PICK_MAX_HITS == SPLAT_PICK_MAX_HITS, "the ABI's limits");
static_assert(PICK_MAX_PIXELS <= 256, "the queries are staged by one workgroup, one per thread");
static_assert(sizeof(splat_pick_result) == 32 && sizeof(splat_pick_layer) == 16 && sizeof(splat_pick_query) == 16, "ABI layouts");

// one Gaussian under the view: visible, and the alpha of its fragment at pixel (x, y) -- 0: none.  The hits kernel and the
// front kernel's second look at a front Gaussian both come through here: the same code, the same bits.
struct PickRecord { float cx, cy; int r[4]; SelProjected m; float opacity; };
template <bool CORRECTED>
static __device__ __forceinline__ bool pick_project(const SelectView& fc, uint64_t n, const float4* __restrict__ planes, uint64_t j,
                                                    const float4& p0, PickRecord* rec) {
    const float4 c0 = planes[n + j], c1 = planes[2 * n + j];
    const float c8 = planes[3 * n + j].x;
    const float c9[9] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c8};
    rec->r[0] = 1; rec->r[1] = 0; rec->r[2] = 1; rec->r[3] = 0;
    rec->opacity = p0.w;
    return sel_project<CORRECTED>(fc, p0.x, p0.y, p0.z, c9, &rec->cx, &rec->cy, rec->r, &rec->m);
}
static __device__ __forceinline__ float pick_alpha_at(const SelectView& fc, const PickRecord& rec, int x, int y) {
    if (x < rec.r[0] || x > rec.r[1] || y < rec.r[2] || y > rec.r[3]) return 0.0f;
    const float off = fc.sample_half ? 0.5f : 0.0f;
    return pick_fragment((float)x + off, (float)y + off, rec.cx, rec.cy, rec.m.hx, rec.m.hy, rec.m.ca, rec.m.cb, rec.m.cc, rec.opacity,
                         fc.y_up != 0);
}

// ---------------------------------------------------------------------------
// The hits.  The queries and the rectangle that bounds them are staged in LDS; thread j judges slot j: plane 0, the caller's
// byte at mask[orig[j]], one projection, the bounding rectangle, then the queries one by one -- every lane reads the same
// query (LDS broadcast) and evaluates the fragment where the pixel lies in its covered range.  A hit costs three atomics,
// all on words of its pixel: the counter hands out its place in the list (the compiler folds the lanes of a wave that hit
// the same pixel into one add), the front key takes the maximum, and the first max_hits places are stored.  The order of a
// list is whatever the atomics made it: the resolve kernel sorts it, and the keys are distinct, so the result is one.
// ---------------------------------------------------------------------------
template <bool CORRECTED>
__global__ __launch_bounds__(256) void pick_hits_kernel(uint64_t n, const float4* __restrict__ planes, const unsigned int* __restrict__ orig,
                                                        const unsigned char* __restrict__ mask, SelectView fc, unsigned int n_pixels,
                                                        const int2* __restrict__ pixels, int4 bound, float alpha_min, unsigned int max_hits,
                                                        unsigned int* __restrict__ counts, unsigned long long* __restrict__ fronts,
                                                        unsigned long long* __restrict__ list_key, float* __restrict__ list_alpha) {
    __shared__ int2 qpix[PICK_MAX_PIXELS];
    __shared__ int4 qbound;
    if (threadIdx.x < n_pixels) qpix[threadIdx.x] = pixels[threadIdx.x];
    if (threadIdx.x == 0) qbound = bound;
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;                                        // (no barrier below)
    const float4 p0 = planes[j];                               // x y z | opacity
    const unsigned int index = orig[j];
    if (mask && mask[index] == 0) return;
    PickRecord rec;
    if (!pick_project<CORRECTED>(fc, n, planes, j, p0, &rec)) return;
    const int4 b = qbound;                                     // x0 y0 x1 y1 of all the queries
    if (rec.r[0] > b.z || rec.r[1] < b.x || rec.r[2] > b.w || rec.r[3] < b.y) return;
    const unsigned long long key = pick_key(rec.m.z, index);
    for (unsigned int q = 0; q < n_pixels; ++q) {
        const int2 p = qpix[q];
        const float alpha = pick_alpha_at(fc, rec, p.x, p.y);
        if (alpha == 0.0f || !(alpha >= alpha_min)) continue;
        const unsigned int place = atomicAdd(&counts[q], 1u);
        atomicMax(&fronts[q], key);
        if (place < max_hits) {
            list_key[(size_t)q * max_hits + place] = key;
            list_alpha[(size_t)q * max_hits + place] = alpha;
        }
    }
}

// ---------------------------------------------------------------------------
// The answer.  Workgroup q holds pixel q: its list (at most max_hits <= 4096 entries of 8 + 4 bytes: 48 KB of LDS) is padded
// to a power of two with key 0 -- below every hit's key -- and put in descending key order by a bitonic network, one
// compare-exchange per thread and step.  Thread 0 then walks the chain (splat_pick_math.h) until the surface is found and
// the layers asked for have their coverage, or to the end when no hit reaches coverage_min; the other threads write the
// rest of the layer rows.  A pixel with more hits than max_hits has no list to speak of: its count and its front are exact
// (neither needed one), its front's alpha is left to pick_front_kernel, and it gets no surface and no layer row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pick_resolve_kernel(float coverage_min, unsigned int max_hits, unsigned int max_layers,
                                                           const unsigned int* __restrict__ counts, const unsigned long long* __restrict__ fronts,
                                                           const unsigned long long* __restrict__ list_key, const float* __restrict__ list_alpha,
                                                           splat_pick_result* __restrict__ results, splat_pick_layer* __restrict__ layers) {
    __shared__ unsigned long long skey[PICK_MAX_HITS];
    __shared__ float salpha[PICK_MAX_HITS];
    const unsigned int q = blockIdx.x, tid = threadIdx.x;
    const unsigned int cnt = counts[q];                        // (uniform)
    splat_pick_result res;
    res.n_hits = cnt; res.flags = 0u;
    res.front_index = SPLAT_PICK_NONE; res.front_depth = 0.0f; res.front_alpha = 0.0f;
    res.surface_index = SPLAT_PICK_NONE; res.surface_depth = 0.0f; res.surface_coverage = 0.0f;

    if (cnt > max_hits) {                                      // (uniform) truncated: the front's alpha is pick_front_kernel's to fill in
        if (tid == 0) {
            const unsigned long long fkey = fronts[q];
            res.flags = SPLAT_PICK_TRUNCATED;
            res.front_index = pick_key_index(fkey);
            res.front_depth = pick_key_depth64(fkey);
            results[q] = res;
        }
        return;
    }

    unsigned int pow2 = 1u;
    while (pow2 < cnt) pow2 <<= 1;                             // (cnt <= max_hits <= PICK_MAX_HITS, a power of two)
    for (unsigned int i = tid; i < pow2; i += 256u) {
        const bool live = i < cnt;
        skey[i] = live ? list_key[(size_t)q * max_hits + i] : 0ull;
        salpha[i] = live ? list_alpha[(size_t)q * max_hits + i] : 0.0f;
    }
    __syncthreads();
    for (unsigned int k = 2u; k <= pow2; k <<= 1)              // (uniform)
        for (unsigned int s = k >> 1; s > 0u; s >>= 1) {
            for (unsigned int t = tid; t < (pow2 >> 1); t += 256u) {
                const unsigned int lo = ((t & ~(s - 1u)) << 1) | (t & (s - 1u)), hi = lo | s;
                const bool descending = (lo & k) == 0u;        // the network's first half of every 2k run ends up descending
                const unsigned long long a = skey[lo], b = skey[hi];
                if ((a < b) == descending) {
                    skey[lo] = b; skey[hi] = a;
                    const float fa = salpha[lo], fb = salpha[hi];
                    salpha[lo] = fb; salpha[hi] = fa;
                }
            }
            __syncthreads();
        }

    const unsigned int rows = layers ? min(cnt, max_layers) : 0u;
    splat_pick_layer* const mine = layers ? layers + (size_t)q * max_layers : nullptr;
    if (tid == 0) {
        if (cnt) {
            res.front_index = pick_key_index(skey[0]);
            res.front_depth = pick_key_depth64(skey[0]);
            res.front_alpha = salpha[0];
        }
        float t = 1.0f, coverage = 0.0f;
        bool surfaced = false;
        for (unsigned int k = 0u; k < cnt; ++k) {
            t = pick_transmit(t, salpha[k]);
            coverage = pick_coverage(t);
            if (k < rows) mine[k].coverage = coverage;
            if (!surfaced && coverage >= coverage_min) {
                surfaced = true;
                res.surface_index = pick_key_index(skey[k]);
                res.surface_depth = pick_key_depth64(skey[k]);
                res.surface_coverage = coverage;
            }
            if (surfaced && k + 1u >= rows) break;
        }
        if (!surfaced) res.surface_coverage = coverage;        // no hit reached coverage_min: what all of them cover
        results[q] = res;
    }
    for (unsigned int k = tid; k < rows; k += 256u) {
        mine[k].index = pick_key_index(skey[k]);
        mine[k].depth = pick_key_depth64(skey[k]);
        mine[k].alpha = salpha[k];
    }
}

// ---------------------------------------------------------------------------
// The alpha of a truncated pixel's front.  The front key names a Gaussian by its original index, and only the thread that
// holds its slot can project it again; finding that slot is a look at the whole order, so it is done by the whole grid, one
// thread per slot, behind the resolve kernel: every workgroup first looks for truncated pixels (counts above max_hits) and
// leaves at once when there is none -- the common case costs n / 256 workgroups that read n_pixels counters each.  Otherwise
// the truncated pixels' front indices are staged in LDS, and the thread whose orig[slot] is one of them projects its
// Gaussian with the code the hits kernel ran -- the same bits -- and writes results[q].front_alpha.  (The measurement that
// asked for this kernel: one workgroup searching the order of 1.5 M Gaussians took 1.5 ms, 30 times the hits kernel.)
// ---------------------------------------------------------------------------
template <bool CORRECTED>
__global__ __launch_bounds__(256) void pick_front_kernel(uint64_t n, const float4* __restrict__ planes, const unsigned int* __restrict__ orig,
                                                         SelectView fc, unsigned int n_pixels, const int2* __restrict__ pixels,
                                                         unsigned int max_hits, const unsigned int* __restrict__ counts,
                                                         const unsigned long long* __restrict__ fronts, splat_pick_result* __restrict__ results) {
    __shared__ unsigned int tindex[PICK_MAX_PIXELS];           // the front's original index of every truncated pixel ...
    __shared__ unsigned int tpixel[PICK_MAX_PIXELS];           // ... and which pixel it is
    __shared__ unsigned int wtot[4];
    const unsigned int tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const bool trunc = tid < n_pixels && counts[tid] > max_hits;
    const unsigned long long m = __ballot(trunc);
    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    if (lane == 0u) wtot[w] = (unsigned int)__popcll(m);
    __syncthreads();
    const unsigned int total = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
    if (total == 0u) return;                                   // (uniform)
    unsigned int before = 0u;
    for (unsigned int k = 0u; k < w; ++k) before += wtot[k];
    if (trunc) { tindex[before + rank] = pick_key_index(fronts[tid]); tpixel[before + rank] = tid; }
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * 256u + tid;
    if (j >= n) return;                                        // (no barrier below)
    const unsigned int index = orig[j];
    bool projected = false, visible = false;
    PickRecord rec;
    for (unsigned int t = 0u; t < total; ++t) {
        if (tindex[t] != index) continue;
        if (!projected) { visible = pick_project<CORRECTED>(fc, n, planes, j, planes[j], &rec); projected = true; }
        const unsigned int q = tpixel[t];
        const int2 p = pixels[q];
        results[q].front_alpha = visible ? pick_alpha_at(fc, rec, p.x, p.y) : 0.0f;
    }
}

// ---------------------------------------------------------------------------
// launch wrapper
// ---------------------------------------------------------------------------
void launch_pick(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const unsigned char* mask, const SelectView& v,
                 const splat_pick_query& q, unsigned int n_pixels, const int2* pixels, int4 bound, const PickTemps& t, void* results,
                 void* layers) {
    if (!n_pixels) return;
    const dim3 block(256);
    if (n) {
        const dim3 grid((unsigned int)((n + 255) / 256));
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, s, n, planes, orig, mask, v, n_pixels, pixels, bound, q.alpha_min, q.max_hits, t.counts,
                               t.fronts, t.list_key, t.list_alpha);
        };
        if (v.corrected) go(pick_hits_kernel<true>); else go(pick_hits_kernel<false>);
    }
    hipLaunchKernelGGL(pick_resolve_kernel, dim3(n_pixels), block, 0, s, q.coverage_min, q.max_hits, q.max_layers, (const unsigned int*)t.counts,
                       (const unsigned long long*)t.fronts, (const unsigned long long*)t.list_key, (const float*)t.list_alpha,
                       (splat_pick_result*)results, (splat_pick_layer*)(q.max_layers ? layers : nullptr));
    if (n) {
        const dim3 grid((unsigned int)((n + 255) / 256));
        auto front = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, s, n, planes, orig, v, n_pixels, pixels, q.max_hits, (const unsigned int*)t.counts,
                               (const unsigned long long*)t.fronts, (splat_pick_result*)results);
        };
        if (v.corrected) front(pick_front_kernel<true>); else front(pick_front_kernel<false>);
    }
}

}  // namespace splat
