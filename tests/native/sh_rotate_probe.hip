// sh_rotate_probe.hip -- TEST ONLY.  The sh rotation of one Gaussian (rotate_sh_bands of splat_amd/csrc/splat_sh_math.h)
// behind C entry points, so that tests/test_sh_rotate_math_host.py (the __host__ compile) can hold it to a numpy
// restatement bit for bit and tests/test_gpu_sh_rotate.py (the device compile) can hold the two compiles to each other.
// Built by splat_amd/csrc/Makefile with the product's flags into tests/native/libsh_rotate_probe.so; not linked into
// libsplat_hip.so.
//
// d1, d2, d3: the blocks (9, 25, 49 floats, row-major); sh45: 45 floats per Gaussian, the floats sh[3..48); the results go
// to out, which has sh45's shape.  All host pointers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "splat_sh_math.h"

namespace {

struct DevBuf {                      // freed on every return path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() { return static_cast<T*>(p); }
};
#define CK(x) do { int e_ = (int)(x); if (e_ != 0) return e_; } while (0)
constexpr uint64_t MAX_N = 1ull << 24;

__host__ __device__ inline void one(const SplatShBlocks& b, const float* sh45, float* out) {
    float c[45];
    for (int e = 0; e < 45; ++e) c[e] = sh45[e];
    rotate_sh_bands(b, c);
    for (int e = 0; e < 45; ++e) out[e] = c[e];
}

__global__ void k_rotate_sh(SplatShBlocks b, uint64_t n, const float* __restrict__ sh45, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    one(b, sh45 + 45 * i, out + 45 * i);
}

SplatShBlocks blocks_of(const float* d1, const float* d2, const float* d3) {
    SplatShBlocks b;
    for (int i = 0; i < 9; ++i) b.d1[i] = d1[i];
    for (int i = 0; i < 25; ++i) b.d2[i] = d2[i];
    for (int i = 0; i < 49; ++i) b.d3[i] = d3[i];
    return b;
}

}  // namespace

extern "C" {

int sh_rotate_probe_device(const float* d1, const float* d2, const float* d3, uint64_t n, const float* sh45, float* out) {
    if (n == 0) return 0;
    if (n > MAX_N || !d1 || !d2 || !d3 || !sh45 || !out) return (int)hipErrorInvalidValue;
    const SplatShBlocks b = blocks_of(d1, d2, d3);
    DevBuf di, dout;
    CK(di.alloc(n * 180)); CK(dout.alloc(n * 180));
    CK(hipMemcpy(di.p, sh45, n * 180, hipMemcpyHostToDevice));
    k_rotate_sh<<<(unsigned int)((n + 255u) / 256u), 256>>>(b, n, di.as<float>(), dout.as<float>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, n * 180, hipMemcpyDeviceToHost));
    return 0;
}

// the __host__ compile of the same text: no GPU needed
void sh_rotate_probe_host(const float* d1, const float* d2, const float* d3, uint64_t n, const float* sh45, float* out) {
    const SplatShBlocks b = blocks_of(d1, d2, d3);
    for (uint64_t i = 0; i < n; ++i) one(b, sh45 + 45 * i, out + 45 * i);
}

}  // extern "C"
