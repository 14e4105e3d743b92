// ply_encode_probe.hip -- TEST ONLY.  The four functions of splat_amd/csrc/splat_ply_encode_math.h, and the chain for one
// Gaussian, behind C entry points, so that tests/test_ply_encode_math_host.py (the __host__ compile) can hold them to
// float64 references and tests/test_gpu_ply_encode.py (the device compile) can hold the two compiles, and the product's
// kernel, to each other bit for bit.  Built by splat_amd/csrc/Makefile with the product's flags into
// tests/native/libply_encode_probe.so; not linked into libsplat_hip.so.
//
// which:  0 ply_log     in: 1 f32 (widened to double)        out: 1 f32
//         1 ply_logit   in: 1 f32                            out: 1 f32
//         2 ply_eig3    in: 6 f32 (S00 S01 S02 S11 S12 S22)  out: 12 f64 (lam[3], V[9] with V(r,c) = V[3c + r])
//         3 ply_quat    in: 9 f64 (V)                        out: 4 f32 (i j k w)
//         4 ply_encode_one   in: 10 f32 (cov[9], opacity)    out: 8 f32 (scale_0..2, opacity, rot_1 rot_2 rot_3 rot_0)
// n elements; all host pointers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "splat_ply_encode_math.h"

namespace {

struct DevBuf {                      // freed on every return path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
};
#define CK(x) do { int e_ = (int)(x); if (e_ != 0) return e_; } while (0)
constexpr uint64_t MAX_N = 1ull << 24;
constexpr size_t IN_BYTES[5] = {4, 4, 24, 72, 40}, OUT_BYTES[5] = {4, 4, 96, 16, 32};

__host__ __device__ inline void one(int which, const void* in, void* out) {
    if (which == 0) {
        *(float*)out = ply_log((double)*(const float*)in);
    } else if (which == 1) {
        *(float*)out = ply_logit(*(const float*)in);
    } else if (which == 2) {
        const float* s = (const float*)in;
        const float c6[6] = {s[0], s[1], s[2], s[3], s[4], s[5]};
        double lam[3], V[9];
        ply_eig3(c6, lam, V);
        double* o = (double*)out;
        for (int e = 0; e < 3; ++e) o[e] = lam[e];
        for (int e = 0; e < 9; ++e) o[3 + e] = V[e];
    } else if (which == 3) {
        const double* s = (const double*)in;
        const double V[9] = {s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]};
        float q[4];
        ply_quat(V, q);
        for (int e = 0; e < 4; ++e) ((float*)out)[e] = q[e];
    } else {
        const float* s = (const float*)in;
        const float cov[9] = {s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]};
        float o[8];
        ply_encode_one(cov, s[9], o);
        for (int e = 0; e < 8; ++e) ((float*)out)[e] = o[e];
    }
}

__global__ void k_ply_encode(int which, uint64_t n, size_t in_bytes, size_t out_bytes, const unsigned char* __restrict__ in,
                             unsigned char* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    one(which, in + i * in_bytes, out + i * out_bytes);
}

}  // namespace

extern "C" {

int ply_encode_probe_device(int which, uint64_t n, const void* in, void* out) {
    if (n == 0) return 0;
    if (n > MAX_N || which < 0 || which > 4 || !in || !out) return (int)hipErrorInvalidValue;
    DevBuf di, dout;
    CK(di.alloc(n * IN_BYTES[which])); CK(dout.alloc(n * OUT_BYTES[which]));
    CK(hipMemcpy(di.p, in, n * IN_BYTES[which], hipMemcpyHostToDevice));
    k_ply_encode<<<(unsigned int)((n + 255u) / 256u), 256>>>(which, n, IN_BYTES[which], OUT_BYTES[which], (const unsigned char*)di.p,
                                                             (unsigned char*)dout.p);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, n * OUT_BYTES[which], hipMemcpyDeviceToHost));
    return 0;
}

// the __host__ compile of the same text: no GPU needed
int ply_encode_probe_host(int which, uint64_t n, const void* in, void* out) {
    if (which < 0 || which > 4 || (n && (!in || !out))) return -1;
    for (uint64_t i = 0; i < n; ++i) one(which, (const unsigned char*)in + i * IN_BYTES[which], (unsigned char*)out + i * OUT_BYTES[which]);
    return 0;
}

}  // extern "C"
