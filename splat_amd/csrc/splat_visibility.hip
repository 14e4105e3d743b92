// splat_visibility.hip -- what each Gaussian contributes to a view (splat_visibility_device; gfx950): for every Gaussian, on how
// many pixels of a region it is really seen and how much, occlusion taken into account.
//
//   visibility_kernel   one 256-thread workgroup per 16 x 16 tile that meets the region, one pixel per thread: the tile's list,
//                       in blend order in memory, is walked from its far end -- the near end of the scene -- in chunks staged
//                       in LDS; every thread runs the pick's chain on its pixel (splat_pick_math.h: the same text, the same
//                       bits), the chunk's Gaussians collect count / greatest weight / Q24 weight sum in LDS, and a chunk is
//                       flushed with one set of global INTEGER atomics per (tile, Gaussian)
//
// The lists are a two-pass frame's: K1's counting flavour, the scan, the emit and the sort launches with every list in them
// (bin_view_for_query of splat_api.hip), so a hit has the very record, rectangle and depth order a frame draws with -- and the
// pick reports.  Built with K1's flags (no contraction).  Nothing here is a float atomic: the outputs do not depend on the
// order in which tiles, waves or pixels arrive.
#include "splat_internal.h"
#include "splat_pick_math.h"

namespace splat {

constexpr unsigned int VIS_CHUNK = 256;        // list entries staged at a time: one per thread

// op over the wave on the DPP path (row shifts inside the 16-lane rows, then the two row broadcasts of gfx9), valid in lane 63;
// every lane of the wave must be active.  Both ops here have the identity 0.
template <int CTRL, int ROW_MASK>
static __device__ __forceinline__ int vis_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
template <typename Op>
static __device__ __forceinline__ unsigned int vis_wave_reduce(unsigned int x, Op op) {
    int v = (int)x;
    v = op(v, vis_dpp<0x111, 0xf>(v));     // row_shr:1
    v = op(v, vis_dpp<0x112, 0xf>(v));     // row_shr:2
    v = op(v, vis_dpp<0x114, 0xf>(v));     // row_shr:4
    v = op(v, vis_dpp<0x118, 0xf>(v));     // row_shr:8
    v = op(v, vis_dpp<0x142, 0xa>(v));     // row_bcast:15
    v = op(v, vis_dpp<0x143, 0xc>(v));     // row_bcast:31 -> lane 63 holds the wave
    return (unsigned int)__builtin_amdgcn_readlane(v, 63);
}

// ---------------------------------------------------------------------------
// Workgroup (tx, ty) of the region's tile range holds one tile, thread t the pixel (16 tx + t % 16, 16 ty + t / 16); a pixel
// outside the rectangle, off the target or with a zero byte in the pixel mask is not walked.  A chunk is staged by all 256
// threads -- entry k of the chunk is the list's k-th nearest remaining key: its record's centre, half extents, conic and
// opacity, its covered rectangle and its original index; a Gaussian whose byte of the caller's mask is 0 is staged with an
// empty rectangle, so that it is neither seen nor occluding.  Then every wave walks the chunk on its 64 pixels:
//   alpha = pick_fragment, w = T * alpha, T = pick_transmit(T, alpha), seen = w >= weight_min,
// and where the ballot of `seen` is not empty the wave's count (a popcount), greatest weight and Q24 sum (DPP reductions) go to
// the entry's LDS words with three LDS atomics from one lane: a weight is a non-negative float, so its bits order as its value,
// and a tile's sum is below 256 * 2^24 = 2^32.  A wave stops when every one of its pixels has T < weight_min -- w_k <= T_{k-1},
// so nothing behind that point is seen -- and the workgroup when all four waves have; with weight_min == 0 neither happens.
// ---------------------------------------------------------------------------
struct VisRegion { int x0, y0, x1, y1, tx0, ty0, ntx; };
__global__ __launch_bounds__(256) void visibility_kernel(VisRegion rg, int W, int tiles_x, int y_up, int sample_half, float weight_min,
                                                         const unsigned int* __restrict__ offsets, const unsigned int* __restrict__ lens,
                                                         const unsigned long long* __restrict__ keys, const Rec* __restrict__ recs,
                                                         const ushort4* __restrict__ rect, const unsigned int* __restrict__ orig,
                                                         const unsigned char* __restrict__ mask, const unsigned char* __restrict__ pixel_mask,
                                                         unsigned int* __restrict__ pixels, unsigned int* __restrict__ max_weight,
                                                         unsigned long long* __restrict__ weight_sum) {
    __shared__ float4 sa[VIS_CHUNK];           // cx, cy, hx, hy
    __shared__ float4 sb[VIS_CHUNK];           // conic a, b (the pick's sign), c, opacity
    __shared__ ushort4 srect[VIS_CHUNK];       // px0, px1, py0, py1
    __shared__ unsigned int sorig[VIS_CHUNK];
    __shared__ unsigned int acnt[VIS_CHUNK], amax[VIS_CHUNK], asum[VIS_CHUNK];
    __shared__ unsigned int sdone[4];
    const unsigned int tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int tx = rg.tx0 + (int)(blockIdx.x % (unsigned int)rg.ntx), ty = rg.ty0 + (int)(blockIdx.x / (unsigned int)rg.ntx);
    const unsigned int tile = (unsigned int)(ty * tiles_x + tx);
    const unsigned int len = lens[tile];                       // (uniform)
    if (len == 0u) return;
    const int px = tx * TILE + (int)(tid & 15u), py = ty * TILE + (int)(tid >> 4);
    bool walking = px >= rg.x0 && px <= rg.x1 && py >= rg.y0 && py <= rg.y1;
    if (walking && pixel_mask) walking = pixel_mask[(size_t)py * (size_t)W + (size_t)px] != 0;
    if (!__syncthreads_or(walking ? 1 : 0)) return;            // (uniform)
    const unsigned long long* const list = keys + offsets[tile];
    const float off = sample_half ? 0.5f : 0.0f;
    const float sx = (float)px + off, sy = (float)py + off;
    float T = 1.0f;
    bool wave_done = __ballot(walking) == 0ull;                // (wave-uniform)
    acnt[tid] = 0u; amax[tid] = 0u; asum[tid] = 0u;
    if (lane == 0u) sdone[wave] = wave_done ? 1u : 0u;

    for (unsigned int base = 0u; base < len; base += VIS_CHUNK) {
        const unsigned int cnt = min(VIS_CHUNK, len - base);   // (uniform)
        if (tid < cnt) {
            const unsigned int slot = (unsigned int)list[len - 1u - (base + tid)];    // keys carry slots; the far end is the nearest
            const Rec* const r = recs + slot;
            const float4 b = r->b;
            const unsigned int index = orig[slot];
            sa[tid] = r->a;
            sb[tid] = make_float4(b.x, y_up ? b.y : -b.y, b.z, b.w);                 // K1 folded the y axis's sign into the cross term (exact)
            srect[tid] = (mask && mask[index] == 0) ? make_ushort4(1, 0, 1, 0) : rect[slot];
            sorig[tid] = index;
        }
        __syncthreads();
        if (!wave_done) {
            for (unsigned int k = 0u; k < cnt; ++k) {
                const ushort4 rc = srect[k];
                float alpha = 0.0f;
                if (walking && px >= (int)rc.x && px <= (int)rc.y && py >= (int)rc.z && py <= (int)rc.w) {
                    const float4 a = sa[k], b = sb[k];
                    alpha = pick_fragment(sx, sy, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, y_up != 0);
                }
                const float w = T * alpha;
                const bool seen = alpha != 0.0f && w >= weight_min;
                if (alpha != 0.0f) T = pick_transmit(T, alpha);
                const unsigned long long m = __ballot(seen);
                if (m != 0ull) {                               // (wave-uniform)
                    const unsigned int wbits = seen ? __builtin_bit_cast(unsigned int, w) : 0u;
                    const unsigned int q24 = seen ? (unsigned int)(w * 16777216.0f) : 0u;
                    const unsigned int mx = vis_wave_reduce(wbits, [](int x, int y) { return max(x, y); });
                    const unsigned int sum = vis_wave_reduce(q24, [](int x, int y) { return x + y; });
                    if (lane == 0u) {
                        atomicAdd(&acnt[k], (unsigned int)__popcll(m));
                        atomicMax(&amax[k], mx);
                        atomicAdd(&asum[k], sum);
                    }
                }
                if (__ballot(walking && T >= weight_min) == 0ull) {      // (wave-uniform; never with weight_min == 0: T >= 0)
                    wave_done = true;
                    if (lane == 0u) sdone[wave] = 1u;
                    break;
                }
            }
        }
        __syncthreads();
        if (tid < cnt && acnt[tid] != 0u) {
            const unsigned int index = sorig[tid];
            if (pixels) atomicAdd(&pixels[index], acnt[tid]);
            if (max_weight) atomicMax(&max_weight[index], amax[tid]);
            if (weight_sum) atomicAdd(&weight_sum[index], (unsigned long long)asum[tid]);
            acnt[tid] = 0u; amax[tid] = 0u; asum[tid] = 0u;
        }
        if ((sdone[0] & sdone[1] & sdone[2] & sdone[3]) != 0u) break;    // (uniform: written in front of the barrier above)
    }
}

// ---------------------------------------------------------------------------
// launch wrapper
// ---------------------------------------------------------------------------
void launch_visibility(const VisibilityArgs& a) {
    if (a.x0 > a.x1 || a.y0 > a.y1) return;
    VisRegion rg;
    rg.x0 = a.x0; rg.y0 = a.y0; rg.x1 = a.x1; rg.y1 = a.y1;
    rg.tx0 = a.x0 / TILE; rg.ty0 = a.y0 / TILE; rg.ntx = a.x1 / TILE - rg.tx0 + 1;
    const int nty = a.y1 / TILE - rg.ty0 + 1;
    hipLaunchKernelGGL(visibility_kernel, dim3((unsigned int)(rg.ntx * nty)), dim3(256), 0, a.s, rg, a.W, a.tiles_x, a.y_up, a.sample_half,
                       a.weight_min, a.offsets, a.lens, a.keys, a.recs, a.rect, a.orig, a.mask, a.pixel_mask, a.pixels,
                       (unsigned int*)a.max_weight, a.weight_sum);
}

}  // namespace splat
