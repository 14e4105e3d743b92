// device_math_probe.hip -- TEST ONLY.  Each function of splat_amd/csrc/splat_device_math.h behind a C entry point of
// its own, so that tests/test_gpu_device_math.py and tests/test_device_math_host.py can hold it to a reference input
// by input instead of through frames.  Built by splat_amd/csrc/Makefile with the product's flags into
// tests/native/libdevice_math_probe.so; not linked into libsplat_hip.so.
//
// Every device entry point: allocate, copy the inputs in, launch one kernel that calls the function under test once
// per element, copy back, free, return the first HIP error (0 = success).  Every index is below n by construction.
// The probe_host_* entry points call the __host__ compile of the same text and need no GPU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>

#include "splat_device_math.h"

namespace {

struct DevBuf {                      // freed on every return path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    hipError_t put(const void* src, size_t bytes) {
        hipError_t e = alloc(bytes);
        return (e != hipSuccess || !bytes) ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
    template <class T> T* as() { return static_cast<T*>(p); }
};
#define CK(x) do { int e_ = (int)(x); if (e_ != 0) return e_; } while (0)
inline int finish(void* dst, DevBuf& src, size_t bytes) {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (bytes) CK(hipMemcpy(dst, src.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
inline unsigned int blocks(uint64_t n) { return (unsigned int)((n + 255u) / 256u); }
constexpr uint64_t MAX_N = 1ull << 26;          // per call: the caller walks a larger range in chunks

// which: 0 exp_neg, 1 exp_libm (table in LDS, as the compositor stages it), 2 / 3 exp_neg2 component x / y (the other
// component carries a different argument: the components must not see each other)
__device__ __forceinline__ float exp_which(int which, float x, const unsigned long long* tab) {
    const float other = __uint_as_float(__float_as_uint(x) * 2654435761u);
    switch (which) {
    case 0: return exp_neg(x);
    case 1: return exp_libm(x, tab);
    case 2: return exp_neg2((f2){x, other}).x;
    default: return exp_neg2((f2){other, x}).y;
    }
}
__global__ void k_exp(int which, uint32_t first_bits, const uint32_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ out) {
    __shared__ unsigned long long exptab[32];
    if (threadIdx.x < 32) exptab[threadIdx.x] = EXP2F_TAB[threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = in ? in[i] : first_bits + (uint32_t)i;
    out[i] = __float_as_uint(exp_which(which, __uint_as_float(bits), exptab));
}

// every state 0..255 of one channel through blend(), ia and alpha * colour formed as shade / shade_pair form them.
// pair: 0 blend_channel; 1 / 2 blend_channel2 component x / y (the other component: state 255 - k, colour negated)
__global__ void k_blend(uint64_t n, const float* __restrict__ alpha, const float* __restrict__ colour, int pair,
                        uint8_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n * 256u) return;
    const uint64_t i = t >> 8;
    const float k = (float)(unsigned int)(t & 255u), k2 = 255.0f - k;
    const float al = alpha[i], c = colour[i];
    const float ia = 1.0f - al;
    float r;
    if (pair == 0) r = blend_channel(k, ia, al * c);
    else if (pair == 1) r = blend_channel2((f2){k, k2}, ia, al * (f2){c, -c}).x;
    else r = blend_channel2((f2){k2, k}, ia, al * (f2){-c, c}).y;
    out[t] = (uint8_t)r;
}
__global__ void k_div255(float* out) { out[threadIdx.x] = div255((float)threadIdx.x); }

// pair: 0 fragment_alpha; 1 / 2 fragment_alpha2 component x / y (the other component: the neighbouring tuple;
// the packed form reports no coverage of its own: out_cov is 0)
__global__ void k_fragment(uint64_t n, const float2* __restrict__ sxy, const float4* __restrict__ ra,
                           const float4* __restrict__ rb, int libm, int pair, float* __restrict__ out_alpha,
                           uint8_t* __restrict__ out_cov) {
    __shared__ unsigned long long exptab[32];
    if (threadIdx.x < 32) exptab[threadIdx.x] = EXP2F_TAB[threadIdx.x];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float2 s = sxy[i];
    const float4 a = ra[i], b = rb[i];
    bool cov = false;
    float alpha;
    if (pair == 0) {
        if (libm) alpha = fragment_alpha(s.x, s.y, a, b, [&](float x) { return exp_libm(x, exptab); }, cov);
        else alpha = fragment_alpha(s.x, s.y, a, b, [](float x) { return exp_neg(x); }, cov);
    } else {
        const uint64_t j = ((i ^ 1ull) < n) ? (i ^ 1ull) : i;
        const float2 s2 = sxy[j];
        const float4 a2 = ra[j], b2 = rb[j];
        if (pair == 1) {
            alpha = fragment_alpha2((f2){s.x, s2.x}, (f2){s.y, s2.y}, (f2){a.x, a2.x}, (f2){a.y, a2.y},
                                    make_float4(a.z, a2.z, a.w, a2.w), (f2){b.x, b2.x}, (f2){b.z, b2.z}, (f2){b.y, b2.y},
                                    (f2){b.w, b2.w}).x;
        } else {
            alpha = fragment_alpha2((f2){s2.x, s.x}, (f2){s2.y, s.y}, (f2){a2.x, a.x}, (f2){a2.y, a.y},
                                    make_float4(a2.z, a.z, a2.w, a.w), (f2){b2.x, b.x}, (f2){b2.z, b.z}, (f2){b2.y, b.y},
                                    (f2){b2.w, b.w}).y;
        }
    }
    out_alpha[i] = alpha;
    out_cov[i] = cov ? 1 : 0;
}

__global__ void k_cover(uint64_t n, const float* __restrict__ c, const float* __restrict__ h, const float* __restrict__ lo,
                        const float* __restrict__ hi, const float* __restrict__ off, uint8_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = any_sample_covered(c[i], h[i], lo[i], hi[i], off[i]) ? 1 : 0;
}

template <class F> void host_threads(uint64_t n, int nthreads, F f) {
    nthreads = nthreads < 1 ? 1 : (nthreads > 16 ? 16 : nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([=] { for (uint64_t i = n * t / nthreads, e = n * (t + 1) / nthreads; i < e; ++i) f(i); });
    for (auto& x : th) x.join();
}
inline float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
inline uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

}  // namespace

extern "C" {

int probe_device_count(int* n) { CK(hipGetDeviceCount(n)); return 0; }

// out[i] = bits(f(x_i)); x_i = the float with bits first_bits + i when in_bits is NULL, else in_bits[i]
int probe_exp(int which, uint32_t first_bits, const uint32_t* in_bits, uint64_t n, uint32_t* out) {
    if (n == 0) return 0;
    if (n > MAX_N || which < 0 || which > 3) return (int)hipErrorInvalidValue;
    DevBuf din, dout;
    if (in_bits) CK(din.put(in_bits, n * 4));
    CK(dout.alloc(n * 4));
    k_exp<<<blocks(n), 256>>>(which, first_bits, in_bits ? din.as<uint32_t>() : nullptr, n, dout.as<uint32_t>());
    return finish(out, dout, n * 4);
}

int probe_blend(uint64_t n, const float* alpha, const float* colour, int pair, uint8_t* out /* [n][256] */) {
    if (n == 0) return 0;
    if (n > (MAX_N >> 6) || pair < 0 || pair > 2) return (int)hipErrorInvalidValue;
    DevBuf da, dc, dout;
    CK(da.put(alpha, n * 4)); CK(dc.put(colour, n * 4)); CK(dout.alloc(n * 256));
    k_blend<<<blocks(n * 256), 256>>>(n, da.as<float>(), dc.as<float>(), pair, dout.as<uint8_t>());
    return finish(out, dout, n * 256);
}

int probe_div255(float* out /* [256] */) {
    DevBuf dout;
    CK(dout.alloc(256 * 4));
    k_div255<<<1, 256>>>(dout.as<float>());
    return finish(out, dout, 256 * 4);
}

int probe_fragment(uint64_t n, const float* sxy /* [n][2] */, const float* ra /* [n][4] cx cy hx hy */,
                   const float* rb /* [n][4] A B C opacity */, int libm, int pair, float* out_alpha, uint8_t* out_cov) {
    if (n == 0) return 0;
    if (n > MAX_N || pair < 0 || pair > 2 || (pair && libm)) return (int)hipErrorInvalidValue;
    DevBuf ds, da, db, dal, dcv;
    CK(ds.put(sxy, n * 8)); CK(da.put(ra, n * 16)); CK(db.put(rb, n * 16)); CK(dal.alloc(n * 4)); CK(dcv.alloc(n));
    k_fragment<<<blocks(n), 256>>>(n, ds.as<float2>(), da.as<float4>(), db.as<float4>(), libm, pair, dal.as<float>(), dcv.as<uint8_t>());
    CK(finish(out_alpha, dal, n * 4));
    CK(hipMemcpy(out_cov, dcv.p, n, hipMemcpyDeviceToHost));
    return 0;
}

int probe_cover(uint64_t n, const float* c, const float* h, const float* lo, const float* hi, const float* off, uint8_t* out) {
    if (n == 0) return 0;
    if (n > MAX_N) return (int)hipErrorInvalidValue;
    DevBuf dc, dh, dl, dhi, dof, dout;
    CK(dc.put(c, n * 4)); CK(dh.put(h, n * 4)); CK(dl.put(lo, n * 4)); CK(dhi.put(hi, n * 4)); CK(dof.put(off, n * 4));
    CK(dout.alloc(n));
    k_cover<<<blocks(n), 256>>>(n, dc.as<float>(), dh.as<float>(), dl.as<float>(), dhi.as<float>(), dof.as<float>(), dout.as<uint8_t>());
    return finish(out, dout, n);
}

// ---- the __host__ compile of the same text: no GPU needed ----
void probe_host_exp_libm(uint32_t first_bits, const uint32_t* in_bits, uint64_t n, uint32_t* out, int nthreads) {
    host_threads(n, nthreads, [=](uint64_t i) {
        out[i] = to_bits(exp_libm(from_bits(in_bits ? in_bits[i] : first_bits + (uint32_t)i), EXP2F_TAB_HOST));
    });
}
void probe_host_reject_threshold(uint32_t first_bits, const uint32_t* in_bits, uint64_t n, float* out, int nthreads) {
    host_threads(n, nthreads, [=](uint64_t i) {
        out[i] = reject_threshold(from_bits(in_bits ? in_bits[i] : first_bits + (uint32_t)i));
    });
}
void probe_host_cover(uint64_t n, const float* c, const float* h, const float* lo, const float* hi, const float* off,
                      uint8_t* out, int nthreads) {
    host_threads(n, nthreads, [=](uint64_t i) { out[i] = any_sample_covered(c[i], h[i], lo[i], hi[i], off[i]) ? 1 : 0; });
}
void probe_host_div255(float* out /* [256] */) {
    for (int k = 0; k < 256; ++k) out[k] = div255((float)k);
}

}  // extern "C"
