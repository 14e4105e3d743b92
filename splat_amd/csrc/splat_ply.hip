// splat_ply.hip -- PLY vertex rows in device memory -> the five SoA buffers of a GaussianList (gfx950).
//
//   ply_decode_kernel      set_property, src/gaussians.rs:246-283   (ply_store of host/splat_host.cpp)
//   recentre_sum_kernel    the mean position, :394-400: ONE sequential f32 sum per axis, in index order
//   recentre_sub_kernel    position -= mean, :401-402
//
// The host loader (load_from_ply_soa, host/splat_host.cpp) is the specification, bit for bit: the same libm expf
// (expf_libm_full of splat_device_math.h), IEEE add and divide around it, and a sum that no reduction tree, pairwise
// scheme or atomic may stand in for -- another order of the additions gives other bits.
#include "splat_internal.h"
#include "splat_device_math.h"

namespace splat {

// ---------------------------------------------------------------------------
// Decode.  One workgroup takes `rows` consecutive vertex rows.  Their bytes are staged into LDS by coalesced dword
// loads that begin at the 4-byte-aligned address at or below the run's first byte and end with the dword that holds the
// run's last byte: such a dword shares its 4 KiB page with a byte of the payload, so the loads touch no page the
// payload does not.  Nothing else is assumed about alignment -- the payload begins where the text header ended, the
// stride is what the property list adds up to -- so a float is put together from the two dwords it may straddle.
// The outputs are written as the flat arrays they are (element e of the run's part of pos4, of scales3, ...): every
// store instruction of a wave covers 256 consecutive bytes.
// STAGED = false: a row longer than the staging buffer (a stride above 64 KiB) is read from global memory instead,
// dword by aligned dword in the same way.
// ---------------------------------------------------------------------------
// (PLY_ROWS, PLY_STAGE_DWORDS, PLY_STAGE_BYTES: splat_internal.h -- the encoder stages its rows the same way)
struct PlyOffsets { int o[SPLAT_PLY_SLOTS]; };                 // by value: kernel arguments, read with constant indices only

// the little-endian float at byte `b` of the dword array `w` (w[0] begins at an aligned address)
__device__ __forceinline__ float ply_float_at(const uint32_t* w, uint64_t b) {
    const uint64_t d = b >> 2;
    const unsigned int sh = (unsigned int)b & 3u;
    const uint32_t lo = w[d];
    const uint32_t hi = sh ? w[d + 1] : 0u;                    // (aligned: the next dword may lie beyond the payload's last page)
    return __uint_as_float(__builtin_amdgcn_alignbyte(hi, lo, sh));
}

template <bool STAGED>
__global__ __launch_bounds__(256) void ply_decode_kernel(uint64_t n, unsigned int stride, unsigned int rows, PlyOffsets off,
                                                         const unsigned char* __restrict__ d_rows, float* __restrict__ pos4,
                                                         float* __restrict__ scales3, float* __restrict__ opacity,
                                                         float* __restrict__ rot4, float* __restrict__ sh) {
    __shared__ uint32_t stage[STAGED ? PLY_STAGE_DWORDS + 1 : 1];
    __shared__ int slot_off[64];
    const unsigned int t = threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < SPLAT_PLY_SLOTS; ++k) slot_off[k] = off.o[k];
    }
    const uint64_t row0 = (uint64_t)blockIdx.x * rows;
    if (row0 >= n) return;                                     // (uniform; the grid is ceil(n / rows))
    const unsigned int cnt = (unsigned int)((n - row0 < (uint64_t)rows) ? (n - row0) : (uint64_t)rows);
    const unsigned char* first = d_rows + row0 * (uint64_t)stride;
    const unsigned int mis = (unsigned int)((uintptr_t)first & 3u);
    const uint32_t* aligned = (const uint32_t*)(first - mis);
    const uint32_t* w = aligned;
    if (STAGED) {
        const unsigned int dwords = (mis + cnt * stride + 3u) >> 2;        // <= PLY_STAGE_DWORDS: rows * stride <= PLY_STAGE_BYTES
        for (unsigned int d = t; d < dwords; d += 256u) stage[d] = aligned[d];
        w = stage;
    }
    __syncthreads();
    // byte of the run's dword array at which slot k of row r begins; absent slots answer < 0
    auto value = [&](unsigned int r, int k, float absent) -> float {
        const int o = slot_off[k];
        return o >= 0 ? ply_float_at(w, (uint64_t)mis + (uint64_t)r * stride + (unsigned int)o) : absent;
    };
    auto present = [&](int k) { return slot_off[k] >= 0; };
    for (unsigned int e = t; e < cnt * 4u; e += 256u) {        // x y z 1
        const unsigned int r = e >> 2, c = e & 3u;
        pos4[row0 * 4u + e] = c < 3u ? value(r, SPLAT_PLY_SLOT_POS + (int)c, 0.0f) : 1.0f;
    }
    for (unsigned int e = t; e < cnt * 3u; e += 256u) {        // exp(scale_k); an absent scale is 0, not exp(0)
        const unsigned int r = e / 3u, c = e - 3u * r;
        const int k = SPLAT_PLY_SLOT_SCALE + (int)c;
        scales3[row0 * 3u + e] = present(k) ? expf_libm_full(value(r, k, 0.0f)) : 0.0f;
    }
    for (unsigned int e = t; e < cnt; e += 256u)
        opacity[row0 + e] = present(SPLAT_PLY_SLOT_OPACITY) ? sigmoid_libm(value(e, SPLAT_PLY_SLOT_OPACITY, 0.0f)) : 0.0f;
    for (unsigned int e = t; e < cnt * 4u; e += 256u) {        // (i, j, k, w) = rot_1 rot_2 rot_3 rot_0; identity where absent
        const unsigned int r = e >> 2, c = e & 3u;
        rot4[row0 * 4u + e] = value(r, SPLAT_PLY_SLOT_ROT + (int)c, c == 3u ? 1.0f : 0.0f);
    }
    for (unsigned int e = t; e < cnt * 48u; e += 256u) {       // f_dc then f_rest, as stored
        const unsigned int r = e / 48u, c = e - 48u * r;
        sh[row0 * 48u + e] = value(r, SPLAT_PLY_SLOT_SH + (int)c, 0.0f);
    }
}

// ---------------------------------------------------------------------------
// The mean.  ax = 0; for i in 0..n: ax += x[i] -- and likewise y, z -- is a chain of n dependent f32 additions per
// axis; the three chains run side by side in lanes 0..2 of the workgroup's first wave.  Everything else only feeds
// them: all 256 threads fetch chunk c + 1 (coalesced float4 loads, held in registers across the walk of chunk c) and
// then lay it into the other half of a double-buffered LDS array, one row per axis, so that a chain lane reads its
// next values four at a time (ds_read_b128), sixteen in a batch ahead of the sixteen additions that depend on each
// other.  Past the end a chunk is padded with -0.0f, the one value s + v == s holds for with every s, bit for bit.
// Then mean = sum / (float)n, as the host divides.
// ---------------------------------------------------------------------------
constexpr unsigned int SUM_CHUNK = 2048;                       // positions per chunk: 2 buffers x 3 axes x 8 KiB = 48 KiB of LDS
constexpr unsigned int SUM_PER_THREAD = SUM_CHUNK / 256;

__global__ __launch_bounds__(256) void recentre_sum_kernel(uint64_t n, const float4* __restrict__ pos4, float* __restrict__ mean) {
    __shared__ float4 buf[2][3][SUM_CHUNK / 4];
    const unsigned int t = threadIdx.x;
    const uint64_t chunks = (n + SUM_CHUNK - 1) / SUM_CHUNK;
    float4 held[SUM_PER_THREAD];
    bool past[SUM_PER_THREAD];
    auto fetch = [&](uint64_t c) {
#pragma unroll
        for (unsigned int j = 0; j < SUM_PER_THREAD; ++j) {
            const uint64_t i = c * SUM_CHUNK + j * 256u + t;
            held[j] = pos4[i < n ? i : n - 1];                 // (always a load of the array: no branch, no wait in front of the walk)
            past[j] = i >= n;
        }
    };
    auto lay = [&](unsigned int b) {
        float* bx = (float*)buf[b][0]; float* by = (float*)buf[b][1]; float* bz = (float*)buf[b][2];
#pragma unroll
        for (unsigned int j = 0; j < SUM_PER_THREAD; ++j) {
            bx[j * 256u + t] = past[j] ? -0.0f : held[j].x; by[j * 256u + t] = past[j] ? -0.0f : held[j].y;
            bz[j * 256u + t] = past[j] ? -0.0f : held[j].z;
        }
    };
    float acc = 0.0f;
    if (chunks) { fetch(0); lay(0); }
    __syncthreads();
    for (uint64_t c = 0; c < chunks; ++c) {
        const unsigned int b = (unsigned int)c & 1u;
        if (c + 1 < chunks) fetch(c + 1);                      // in flight under the walk
        if (t < 3u) {
            const float4* row = buf[b][t];
            for (unsigned int q = 0; q < SUM_CHUNK / 4; q += 4) {
                const float4 v0 = row[q], v1 = row[q + 1], v2 = row[q + 2], v3 = row[q + 3];
                acc += v0.x; acc += v0.y; acc += v0.z; acc += v0.w;
                acc += v1.x; acc += v1.y; acc += v1.z; acc += v1.w;
                acc += v2.x; acc += v2.y; acc += v2.z; acc += v2.w;
                acc += v3.x; acc += v3.y; acc += v3.z; acc += v3.w;
            }
        }
        if (c + 1 < chunks) lay(b ^ 1u);                       // (the half walked one iteration ago: everyone passed the barrier since)
        __syncthreads();
    }
    if (t < 3u) mean[t] = acc / (float)n;
}

__global__ __launch_bounds__(256) void recentre_sub_kernel(uint64_t n, float4* __restrict__ pos4, const float* __restrict__ mean) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 p = pos4[i];
    p.x -= mean[0]; p.y -= mean[1]; p.z -= mean[2];
    pos4[i] = p;
}

// ---------------------------------------------------------------------------
// launch wrapper: decode, sum, subtract on `s`; ev (nullable): four events recorded around the three kernels
// ---------------------------------------------------------------------------
void launch_ply_decode(hipStream_t s, const splat_ply_layout& lay, const void* d_rows, float* pos4, float* scales3,
                       float* opacity, float* rot4, float* sh, float* mean, hipEvent_t* ev) {
    const uint64_t n = lay.n;
    if (!n) return;
    PlyOffsets off;
    for (int k = 0; k < SPLAT_PLY_SLOTS; ++k) off.o[k] = lay.offset[k];
    const unsigned int fit = PLY_STAGE_BYTES / lay.stride;     // rows whose bytes fit the staging buffer
    const unsigned int rows = fit ? (fit < PLY_ROWS ? fit : PLY_ROWS) : PLY_ROWS;
    const unsigned int grid = (unsigned int)((n + rows - 1) / rows);
    if (ev) (void)hipEventRecord(ev[0], s);
    if (fit)
        hipLaunchKernelGGL(ply_decode_kernel<true>, dim3(grid), dim3(256), 0, s, n, lay.stride, rows, off, (const unsigned char*)d_rows,
                           pos4, scales3, opacity, rot4, sh);
    else
        hipLaunchKernelGGL(ply_decode_kernel<false>, dim3(grid), dim3(256), 0, s, n, lay.stride, rows, off, (const unsigned char*)d_rows,
                           pos4, scales3, opacity, rot4, sh);
    if (ev) (void)hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(recentre_sum_kernel, dim3(1), dim3(256), 0, s, n, (const float4*)pos4, mean);
    if (ev) (void)hipEventRecord(ev[2], s);
    hipLaunchKernelGGL(recentre_sub_kernel, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, n, (float4*)pos4, (const float*)mean);
    if (ev) (void)hipEventRecord(ev[3], s);
}

}  // namespace splat
