// splat_ply_encode.hip -- the resident scene as PLY vertex rows in device memory (splat_encode_ply_scene_device,
// splat_encode_ply_gaussians_device; gfx950): ply_decode_kernel of splat_ply.hip run backwards.
//
//   ply_encode_kernel<INDEXED>   one Gaussian a thread: its slot of the packed planes -> the float32 properties of one row
//
// The arithmetic -- covariance -> three log scales and a quaternion, opacity -> its logit -- is splat_ply_encode_math.h, the
// specification: tests/native/ply_encode_probe.hip compiles the same text for the host, and the rows written here are that
// compile's rows bit for bit.  Positions and the 48 sh floats leave with the bits the planes hold (the resident order is
// f_dc then f_rest already: no transpose); the w of a position is no property.
//
// Unlike the decoder this kernel has no unstaged flavour: a row must fit the stage (stride <= PLY_STAGE_BYTES), and the
// output is whole dwords -- d_rows, the stride and every present offset are multiples of 4 (the entry points refuse
// anything else) -- so that a workgroup owns every dword it stores and two workgroups never share one.
#include "splat_internal.h"
#include "splat_ply_encode_math.h"

namespace splat {

struct PlyEncodeOffsets { int o[SPLAT_PLY_SLOTS]; };           // by value: kernel arguments, read with constant indices only

// ---------------------------------------------------------------------------
// One workgroup takes `rows` consecutive output rows (rows * stride <= PLY_STAGE_BYTES).  Their image is zeroed in LDS --
// what no slot names (nx ny nz, padding) is written as 0 -- then thread t lays the present slots of row row0 + t into it at
// offset[k], and after a barrier the image leaves as the flat dword array it is: every store instruction of a wave covers
// 256 consecutive bytes.
// INDEXED = false: row r is Gaussian r (rows_total == n), read from slot inv[r].
// INDEXED = true:  row r is Gaussian index[r] (rows_total == k), read from slot inv[index[r]]: any order, duplicates allowed.
// The indices arrive checked (launch_index_check).  The eigen-decomposition runs only where a scale or a rot slot is
// present, the logit only where opacity is (uniform branches on kernel arguments).
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(256) void ply_encode_kernel(uint64_t n, uint64_t rows_total, unsigned int stride, unsigned int rows,
                                                         PlyEncodeOffsets off, const unsigned int* __restrict__ index,
                                                         const unsigned int* __restrict__ inv, const float4* __restrict__ planes,
                                                         uint32_t* __restrict__ d_rows) {
    __shared__ uint32_t stage[PLY_STAGE_BYTES / 4];
    const unsigned int t = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * rows;
    if (row0 >= rows_total) return;                            // (uniform; the grid is ceil(rows_total / rows))
    const unsigned int cnt = (unsigned int)((rows_total - row0 < (uint64_t)rows) ? (rows_total - row0) : (uint64_t)rows);
    const unsigned int sd = stride >> 2;                       // dwords per row
    const unsigned int dwords = cnt * sd;                      // <= PLY_STAGE_BYTES / 4
    for (unsigned int d = t; d < dwords; d += 256u) stage[d] = 0u;
    __syncthreads();
    if (t < cnt) {
        const uint64_t r = row0 + t;
        const uint64_t j = inv[INDEXED ? index[r] : (unsigned int)r];
        uint32_t* row = stage + t * sd;
        auto put = [&](int k, float v) {                       // (k is a constant after unrolling: off.o[k] is an SGPR)
            const int o = off.o[k];
            if (o >= 0) row[(unsigned int)o >> 2] = __float_as_uint(v);
        };
        const float4 p0 = planes[j], p3 = planes[3 * n + j];
        put(SPLAT_PLY_SLOT_POS, p0.x); put(SPLAT_PLY_SLOT_POS + 1, p0.y); put(SPLAT_PLY_SLOT_POS + 2, p0.z);
        put(SPLAT_PLY_SLOT_SH, p3.y); put(SPLAT_PLY_SLOT_SH + 1, p3.z); put(SPLAT_PLY_SLOT_SH + 2, p3.w);
#pragma unroll
        for (int p = 4; p < 15; ++p) {                         // plane p: sh[4p - 13 .. 4p - 10]
            const float4 v = planes[(uint64_t)p * n + j];
            const int k = SPLAT_PLY_SLOT_SH + 4 * p - 13;
            put(k, v.x); put(k + 1, v.y); put(k + 2, v.z); put(k + 3, v.w);
        }
        put(SPLAT_PLY_SLOT_SH + 47, planes[15 * n + j].x);
        if (off.o[SPLAT_PLY_SLOT_OPACITY] >= 0) put(SPLAT_PLY_SLOT_OPACITY, ply_logit(p0.w));
        bool shape = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) shape = shape || off.o[SPLAT_PLY_SLOT_SCALE + k] >= 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) shape = shape || off.o[SPLAT_PLY_SLOT_ROT + k] >= 0;
        if (shape) {
            const float4 c0 = planes[n + j], c1 = planes[2 * n + j];
            const float c6[6] = {c0.x, c0.w, c1.z, c1.x, c1.w, p3.x};      // S00 S01 S02 S11 S12 S22 of cov[3c + r]
            double lam[3], V[9];
            float q[4];
            ply_eig3(c6, lam, V);
            ply_quat(V, q);
#pragma unroll
            for (int k = 0; k < 3; ++k) put(SPLAT_PLY_SLOT_SCALE + k, ply_log(lam[k]));
#pragma unroll
            for (int k = 0; k < 4; ++k) put(SPLAT_PLY_SLOT_ROT + k, q[k]);
        }
    }
    __syncthreads();
    uint32_t* out = d_rows + row0 * sd;
    for (unsigned int d = t; d < dwords; d += 256u) out[d] = stage[d];
}

// ---------------------------------------------------------------------------
// launch wrapper.  The layout arrives checked (stride a multiple of 4 in [4, PLY_STAGE_BYTES], offsets multiples of 4 inside
// the row or -1); index == nullptr: the whole scene, rows_total == n.
// ---------------------------------------------------------------------------
void launch_ply_encode(hipStream_t s, uint64_t n, uint64_t rows_total, const unsigned int* index, const splat_ply_layout& lay,
                       const unsigned int* inv, const float4* planes, void* d_rows) {
    if (!rows_total) return;
    PlyEncodeOffsets off;
    for (int k = 0; k < SPLAT_PLY_SLOTS; ++k) off.o[k] = lay.offset[k];
    const unsigned int fit = PLY_STAGE_BYTES / lay.stride;     // >= 1
    const unsigned int rows = fit < PLY_ROWS ? fit : PLY_ROWS;
    const unsigned int grid = (unsigned int)((rows_total + rows - 1) / rows);
    if (index)
        hipLaunchKernelGGL(ply_encode_kernel<true>, dim3(grid), dim3(256), 0, s, n, rows_total, lay.stride, rows, off, index, inv, planes,
                           (uint32_t*)d_rows);
    else
        hipLaunchKernelGGL(ply_encode_kernel<false>, dim3(grid), dim3(256), 0, s, n, rows_total, lay.stride, rows, off, index, inv, planes,
                           (uint32_t*)d_rows);
}

}  // namespace splat
