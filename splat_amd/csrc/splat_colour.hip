// splat_colour.hip -- the colour tools of the resident scene (splat_eval_colours_device, splat_select_colour_device,
// splat_recolour_scene_device, splat_recolour_gaussians_device; gfx950).
//
//   eval_colour_kernel<INDEXED>   the colour a Gaussian is drawn with under a camera: three floats a row
//   select_colour_kernel          the same colour judged by a query in colour space, combined with the caller's byte at
//                                 selection[orig[slot]], and the count of what is selected afterwards
//   recolour_kernel<INDEXED>      a 3x4 map of the colour applied to the sh coefficients of a Gaussian, in place on the planes;
//                                 everything else keeps its bits
//
// The colour is the colour half of K1 (preprocess_kernel of splat_kernels.hip) restated (splat_colour_math.h): the same f32
// operations in the same order, built with the same flags -- no contraction, correctly rounded division and square root --
// so the same bits (tests/test_gpu_colour.py holds it to the oracle).  All three are memory bound, one thread per slot or
// row, and need no LDS beyond the selection's count.  The inverse of the order and the index check are splat_update.hip's.
#include "splat_internal.h"
#include "splat_colour_math.h"

namespace splat {

struct ColourView { float cam[3]; int sh_dim; };   // what the colour needs of a camera (a kernel argument by value: SGPRs)

// ---------------------------------------------------------------------------
// The colour of slot j.  Plane 0 holds x y z | opacity, plane 3 cov[8] | sh0 sh1 sh2, plane p (4 <= p <= 14)
// sh[4p - 13 .. 4p - 10], plane 15 sh[47] in .x.  sh_dim is uniform, so the planes of a band that is not evaluated are not
// loaded, as in K1: band 1 ends in plane 6, band 2 in plane 9, band 3 takes the rest -- 32, 80, 128 or 224 bytes a Gaussian.
// Every index into sh[] is a constant after unrolling: the values live in registers.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void slot_colour(const float4* __restrict__ planes, uint64_t n, uint64_t j, const ColourView& v, float rgb[3]) {
    float sh[48];
    const float4 p0 = planes[j], p3 = planes[3 * n + j];
    sh[0] = p3.y; sh[1] = p3.z; sh[2] = p3.w;
    auto load = [&](int p) {
        const float4 t = planes[(uint64_t)p * n + j];
        sh[4 * p - 13] = t.x; sh[4 * p - 12] = t.y; sh[4 * p - 11] = t.z; sh[4 * p - 10] = t.w;
    };
    if (v.sh_dim > 3) {
#pragma unroll
        for (int p = 4; p < 7; ++p) load(p);
        if (v.sh_dim > 12) {
#pragma unroll
            for (int p = 7; p < 10; ++p) load(p);
            if (v.sh_dim > 27) {
#pragma unroll
                for (int p = 10; p < 15; ++p) load(p);
                sh[47] = planes[15 * n + j].x;
            }
        }
    }
    const float pos[3] = {p0.x, p0.y, p0.z};
    colour_under_camera(pos, v.cam, v.sh_dim, sh, rgb);
}

// INDEXED = false: thread j judges slot j and writes row orig[j] (rows == n).
// INDEXED = true:  thread t judges slot inv[index[t]] and writes row t (rows == k); an index named twice gives two rows.
template <bool INDEXED>
__global__ __launch_bounds__(256)
void eval_colour_kernel(uint64_t n, uint64_t rows, ColourView v, const unsigned int* __restrict__ orig,
                        const unsigned int* __restrict__ index, const unsigned int* __restrict__ inv,
                        const float4* __restrict__ planes, float* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= rows) return;
    uint64_t j, r;                                             // the slot read, the row written
    if (INDEXED) { r = t; j = inv[index[t]]; } else { j = t; r = orig[t]; }
    float rgb[3];
    slot_colour(planes, n, j, v, rgb);
    out[3 * r] = rgb[0]; out[3 * r + 1] = rgb[1]; out[3 * r + 2] = rgb[2];
}

// The op on the caller's byte and the count are select_kernel's (splat_select.hip): the byte of a Gaussian belongs to the one
// thread that holds its slot (orig is a permutation), so nothing races; a ballot and a popcount per wave, the four summed in
// LDS, one atomic per workgroup that selected any.
__global__ __launch_bounds__(256)
void select_colour_kernel(uint64_t n, const float4* __restrict__ planes, const unsigned int* __restrict__ orig, splat_colour_query q,
                          ColourView v, uint32_t op, unsigned char* selection, unsigned int* __restrict__ count) {
    __shared__ unsigned int wsel[4];
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool sel = false;
    if (j < n) {
        float rgb[3];
        slot_colour(planes, n, j, v, rgb);
        const bool pass = colour_passes(q, rgb);
        unsigned char* const b = selection + orig[j];
        if (op == SPLAT_SEL_OP_SET) { sel = pass; *b = (unsigned char)(pass ? 1 : 0); }
        else {
            const bool old = *b != 0;
            if (op == SPLAT_SEL_OP_ADD) { sel = old || pass; if (pass) *b = (unsigned char)1; }
            else if (op == SPLAT_SEL_OP_SUBTRACT) { sel = old && !pass; if (pass) *b = (unsigned char)0; }
            else { sel = old && pass; *b = (unsigned char)(sel ? 1 : 0); }
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
// Recolour.  sh[0..48) of slot j lies in planes 3-15: thirteen float4 loads, the sixteen 3x3 products of
// splat_colour_math.h (144 multiplies and their adds on 48 register-resident values), thirteen float4 stores -- 416 bytes a
// Gaussian.  Plane 3's .x (cov[8]) and plane 15's .yzw go back as they came.  The twelve floats of the map are a by-value
// argument.  Positions and covariances stay, so no block bounds change and nothing is marked dirty.  A slot belongs to one
// thread (the indices are distinct), so nothing races.
// INDEXED = false: thread j maps slot j (rows == n).  INDEXED = true: thread t maps slot inv[index[t]] (rows == k).
// ---------------------------------------------------------------------------
template <bool INDEXED>
__global__ __launch_bounds__(256)
void recolour_kernel(uint64_t n, uint64_t rows, SplatColourMap m, const unsigned int* __restrict__ index,
                     const unsigned int* __restrict__ inv, float4* __restrict__ planes) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= rows) return;
    const uint64_t j = INDEXED ? (uint64_t)inv[index[t]] : t;
    float4 v[13];
#pragma unroll
    for (int p = 0; p < 13; ++p) v[p] = planes[(uint64_t)(p + 3) * n + j];
    float c[48];
    c[0] = v[0].y; c[1] = v[0].z; c[2] = v[0].w;
#pragma unroll
    for (int p = 1; p < 12; ++p) { c[4 * p - 1] = v[p].x; c[4 * p] = v[p].y; c[4 * p + 1] = v[p].z; c[4 * p + 2] = v[p].w; }
    c[47] = v[12].x;
    recolour_coefficients(m, c);
    // (the floats that stay are named one by one: a float4 handed on whole travels through a 12-byte copy in LDS)
    const float cov8 = v[0].x, y15 = v[12].y, z15 = v[12].z, w15 = v[12].w;
    planes[3 * n + j] = make_float4(cov8, c[0], c[1], c[2]);
#pragma unroll
    for (int p = 1; p < 12; ++p) planes[(uint64_t)(p + 3) * n + j] = make_float4(c[4 * p - 1], c[4 * p], c[4 * p + 1], c[4 * p + 2]);
    planes[15 * n + j] = make_float4(c[47], y15, z15, w15);
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
static inline unsigned int colour_blocks(uint64_t n) { return (unsigned int)((n + 255) / 256); }
static inline ColourView colour_view(const float cam_pos[3], int sh_dim) {
    ColourView v;
    for (int a = 0; a < 3; ++a) v.cam[a] = cam_pos[a];
    v.sh_dim = sh_dim;
    return v;
}

void launch_eval_colours_scene(hipStream_t s, uint64_t n, const float cam_pos[3], int sh_dim, const unsigned int* orig,
                               const float4* planes, float* out) {
    if (!n) return;
    hipLaunchKernelGGL(eval_colour_kernel<false>, dim3(colour_blocks(n)), dim3(256), 0, s, n, n, colour_view(cam_pos, sh_dim), orig,
                       (const unsigned int*)nullptr, (const unsigned int*)nullptr, planes, out);
}

void launch_eval_colours_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const float cam_pos[3], int sh_dim,
                                 const unsigned int* inv, const float4* planes, float* out) {
    if (!k) return;
    hipLaunchKernelGGL(eval_colour_kernel<true>, dim3(colour_blocks(k)), dim3(256), 0, s, n, k, colour_view(cam_pos, sh_dim),
                       (const unsigned int*)nullptr, index, inv, planes, out);
}

void launch_select_colour(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const splat_colour_query& q,
                          const float cam_pos[3], int sh_dim, uint32_t op, unsigned char* selection, unsigned int* count) {
    if (!n) return;
    hipLaunchKernelGGL(select_colour_kernel, dim3(colour_blocks(n)), dim3(256), 0, s, n, planes, orig, q, colour_view(cam_pos, sh_dim), op,
                       selection, count);
}

void launch_recolour_scene(hipStream_t s, uint64_t n, const SplatColourMap& m, float4* planes) {
    if (!n) return;
    hipLaunchKernelGGL(recolour_kernel<false>, dim3(colour_blocks(n)), dim3(256), 0, s, n, n, m, (const unsigned int*)nullptr,
                       (const unsigned int*)nullptr, planes);
}

void launch_recolour_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const SplatColourMap& m,
                             const unsigned int* inv, float4* planes) {
    if (!k) return;
    hipLaunchKernelGGL(recolour_kernel<true>, dim3(colour_blocks(k)), dim3(256), 0, s, n, k, m, index, inv, planes);
}

}  // namespace splat
