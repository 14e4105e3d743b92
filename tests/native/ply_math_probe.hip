// ply_math_probe.hip -- TEST ONLY.  The PLY decoder's two activations (expf_libm_full and sigmoid_libm of
// splat_amd/csrc/splat_device_math.h) behind C entry points, so that tests/test_ply_math_host.py (the __host__ compile)
// and tests/test_gpu_ply_device.py (the device compile) can hold them to glibc's expf argument by argument.  Built by
// splat_amd/csrc/Makefile with the product's flags into tests/native/libply_math_probe.so; not linked into
// libsplat_hip.so.
//
// which: 0 expf_libm_full, 1 sigmoid_libm.  The argument of element i is the float with bits in_bits[i], or, without
// an array, first_bits + i * step (mod 2^32).  Every index is below n by construction.
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
    template <class T> T* as() { return static_cast<T*>(p); }
};
#define CK(x) do { int e_ = (int)(x); if (e_ != 0) return e_; } while (0)
constexpr uint64_t MAX_N = 1ull << 26;          // per call: the caller walks a larger range in chunks

__host__ __device__ inline float ply_which(int which, float x) { return which ? sigmoid_libm(x) : expf_libm_full(x); }

__global__ void k_ply_math(int which, uint32_t first_bits, uint32_t step, const uint32_t* __restrict__ in, uint64_t n,
                           uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = in ? in[i] : first_bits + (uint32_t)i * step;
    out[i] = __float_as_uint(ply_which(which, __uint_as_float(bits)));
}

}  // namespace

extern "C" {

int ply_probe_device(int which, uint32_t first_bits, uint32_t step, const uint32_t* in_bits, uint64_t n, uint32_t* out) {
    if (n == 0) return 0;
    if (n > MAX_N || which < 0 || which > 1) return (int)hipErrorInvalidValue;
    DevBuf din, dout;
    if (in_bits) {
        CK(din.alloc(n * 4));
        CK(hipMemcpy(din.p, in_bits, n * 4, hipMemcpyHostToDevice));
    }
    CK(dout.alloc(n * 4));
    k_ply_math<<<(unsigned int)((n + 255u) / 256u), 256>>>(which, first_bits, step, in_bits ? din.as<uint32_t>() : nullptr, n, dout.as<uint32_t>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the __host__ compile of the same text: no GPU needed
void ply_probe_host(int which, uint32_t first_bits, uint32_t step, const uint32_t* in_bits, uint64_t n, uint32_t* out, int nthreads) {
    nthreads = nthreads < 1 ? 1 : (nthreads > 16 ? 16 : nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([=] {
            for (uint64_t i = n * t / nthreads, e = n * (t + 1) / nthreads; i < e; ++i) {
                const uint32_t b = in_bits ? in_bits[i] : first_bits + (uint32_t)i * step;
                float x; memcpy(&x, &b, 4);
                const float y = ply_which(which, x);
                memcpy(out + i, &y, 4);
            }
        });
    for (auto& x : th) x.join();
}

}  // extern "C"
