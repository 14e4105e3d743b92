// transform_math_probe.hip -- TEST ONLY.  The affine map of one Gaussian (transform_point and transform_cov3d of
// splat_amd/csrc/splat_transform_math.h) behind C entry points, so that tests/test_transform_math_host.py (the __host__
// compile) can hold it to a numpy restatement bit for bit and tests/test_gpu_scene_read.py (the device compile) can hold
// the two compiles to each other.  Built by splat_amd/csrc/Makefile with the product's flags into
// tests/native/libtransform_math_probe.so; not linked into libsplat_hip.so.
//
// m: 12 floats (3x4 row-major); pos: 3 floats per Gaussian; cov: 9 floats per Gaussian (column-major blocks); the results
// go to pos_out and cov_out, which have the inputs' shapes.  All host pointers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "splat_transform_math.h"

namespace {

struct DevBuf {                      // freed on every return path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() { return static_cast<T*>(p); }
};
#define CK(x) do { int e_ = (int)(x); if (e_ != 0) return e_; } while (0)
constexpr uint64_t MAX_N = 1ull << 24;

__host__ __device__ inline void one(const float* m, const float* pos, const float* cov, float* pos_out, float* cov_out) {
    float p[3], c[9];
    transform_point(m, pos[0], pos[1], pos[2], p);
    transform_cov3d(m, cov, c);
    for (int a = 0; a < 3; ++a) pos_out[a] = p[a];
    for (int e = 0; e < 9; ++e) cov_out[e] = c[e];
}

__global__ void k_transform_math(SplatAffine a, uint64_t n, const float* __restrict__ pos, const float* __restrict__ cov,
                                 float* __restrict__ pos_out, float* __restrict__ cov_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    one(a.m, pos + 3 * i, cov + 9 * i, pos_out + 3 * i, cov_out + 9 * i);
}

}  // namespace

extern "C" {

int transform_probe_device(const float* m, uint64_t n, const float* pos, const float* cov, float* pos_out, float* cov_out) {
    if (n == 0) return 0;
    if (n > MAX_N || !m || !pos || !cov || !pos_out || !cov_out) return (int)hipErrorInvalidValue;
    SplatAffine a;
    for (int i = 0; i < 12; ++i) a.m[i] = m[i];
    DevBuf dp, dc, dpo, dco;
    CK(dp.alloc(n * 12)); CK(dc.alloc(n * 36)); CK(dpo.alloc(n * 12)); CK(dco.alloc(n * 36));
    CK(hipMemcpy(dp.p, pos, n * 12, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc.p, cov, n * 36, hipMemcpyHostToDevice));
    k_transform_math<<<(unsigned int)((n + 255u) / 256u), 256>>>(a, n, dp.as<float>(), dc.as<float>(), dpo.as<float>(), dco.as<float>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(pos_out, dpo.p, n * 12, hipMemcpyDeviceToHost));
    CK(hipMemcpy(cov_out, dco.p, n * 36, hipMemcpyDeviceToHost));
    return 0;
}

// the __host__ compile of the same text: no GPU needed
void transform_probe_host(const float* m, uint64_t n, const float* pos, const float* cov, float* pos_out, float* cov_out) {
    for (uint64_t i = 0; i < n; ++i) one(m, pos + 3 * i, cov + 9 * i, pos_out + 3 * i, cov_out + 9 * i);
}

}  // extern "C"
