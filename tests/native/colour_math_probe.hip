// colour_math_probe.hip -- TEST ONLY.  The colour arithmetic of one Gaussian (colour_under_camera, colour_passes,
// recolour_coefficients and recolour_offset of splat_amd/csrc/splat_colour_math.h) behind C entry points over arrays, so that
// tests/test_colour_math_host.py (the __host__ compile) can hold it to a numpy restatement bit for bit and
// tests/test_gpu_colour.py (the device compile) can hold the two compiles to each other.  Built by splat_amd/csrc/Makefile
// with the product's flags into tests/native/libcolour_math_probe.so; not linked into libsplat_hip.so.
//
// pos3: 3 floats per Gaussian; sh48: 48; rgb: 3; pass: one byte (0 / 1).  All host pointers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "splat_colour_math.h"

namespace {

struct DevBuf {                      // freed on every return path
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() { return static_cast<T*>(p); }
};
#define CK(x) do { int e_ = (int)(x); if (e_ != 0) return e_; } while (0)
constexpr uint64_t MAX_N = 1ull << 24;
struct Cam { float pos[3]; };

__host__ __device__ inline void one_eval(const Cam& cam, int sh_dim, const float* pos3, const float* sh48, float* rgb) {
    float sh[48];
    for (int e = 0; e < 48; ++e) sh[e] = sh48[e];
    colour_under_camera(pos3, cam.pos, sh_dim, sh, rgb);
}

__host__ __device__ inline void one_recolour(const SplatColourMap& m, const float* sh48, float* out) {
    float c[48];
    for (int e = 0; e < 48; ++e) c[e] = sh48[e];
    recolour_coefficients(m, c);
    for (int e = 0; e < 48; ++e) out[e] = c[e];
}

__global__ void k_eval(Cam cam, int sh_dim, uint64_t n, const float* __restrict__ pos3, const float* __restrict__ sh48,
                       float* __restrict__ rgb) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    one_eval(cam, sh_dim, pos3 + 3 * i, sh48 + 48 * i, rgb + 3 * i);
}

__global__ void k_passes(splat_colour_query q, uint64_t n, const float* __restrict__ rgb, unsigned char* __restrict__ pass) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    pass[i] = (unsigned char)(colour_passes(q, rgb + 3 * i) ? 1 : 0);
}

__global__ void k_recolour(SplatColourMap m, uint64_t n, const float* __restrict__ sh48, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    one_recolour(m, sh48 + 48 * i, out + 48 * i);
}

SplatColourMap map_of(const float* a9, const float* o3) {
    SplatColourMap m;
    for (int i = 0; i < 9; ++i) m.a[i] = a9[i];
    for (int i = 0; i < 3; ++i) m.o[i] = o3[i];
    return m;
}
Cam cam_of(const float* p) { return Cam{{p[0], p[1], p[2]}}; }
unsigned int blocks(uint64_t n) { return (unsigned int)((n + 255u) / 256u); }

}  // namespace

extern "C" {

// ---- the __host__ compile: no GPU needed ------------------------------------------------------------------------------------
void colour_probe_eval_host(const float* cam_pos, int32_t sh_dim, uint64_t n, const float* pos3, const float* sh48, float* rgb) {
    const Cam cam = cam_of(cam_pos);
    for (uint64_t i = 0; i < n; ++i) one_eval(cam, sh_dim, pos3 + 3 * i, sh48 + 48 * i, rgb + 3 * i);
}

void colour_probe_passes_host(const splat_colour_query* q, uint64_t n, const float* rgb, unsigned char* pass) {
    for (uint64_t i = 0; i < n; ++i) pass[i] = (unsigned char)(colour_passes(*q, rgb + 3 * i) ? 1 : 0);
}

void colour_probe_recolour_host(const float* a9, const float* o3, uint64_t n, const float* sh48, float* out) {
    const SplatColourMap m = map_of(a9, o3);
    for (uint64_t i = 0; i < n; ++i) one_recolour(m, sh48 + 48 * i, out + 48 * i);
}

// o (3 floats) from m (12 floats); returns 1 when recolour_map refuses m, else 0 with a9 filled as well
int colour_probe_map(const float* m12, float* a9, float* o3) {
    recolour_offset(m12, o3);
    SplatColourMap map;
    if (recolour_map(m12, map)) return 1;
    for (int i = 0; i < 9; ++i) a9[i] = map.a[i];
    for (int i = 0; i < 3; ++i) o3[i] = map.o[i];
    return 0;
}

// ---- the device compile of the same text ------------------------------------------------------------------------------------
int colour_probe_eval_device(const float* cam_pos, int32_t sh_dim, uint64_t n, const float* pos3, const float* sh48, float* rgb) {
    if (n == 0) return 0;
    if (n > MAX_N || !cam_pos || !pos3 || !sh48 || !rgb) return (int)hipErrorInvalidValue;
    DevBuf dp, ds, dout;
    CK(dp.alloc(n * 12)); CK(ds.alloc(n * 192)); CK(dout.alloc(n * 12));
    CK(hipMemcpy(dp.p, pos3, n * 12, hipMemcpyHostToDevice));
    CK(hipMemcpy(ds.p, sh48, n * 192, hipMemcpyHostToDevice));
    k_eval<<<blocks(n), 256>>>(cam_of(cam_pos), sh_dim, n, dp.as<float>(), ds.as<float>(), dout.as<float>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(rgb, dout.p, n * 12, hipMemcpyDeviceToHost));
    return 0;
}

int colour_probe_passes_device(const splat_colour_query* q, uint64_t n, const float* rgb, unsigned char* pass) {
    if (n == 0) return 0;
    if (n > MAX_N || !q || !rgb || !pass) return (int)hipErrorInvalidValue;
    DevBuf di, dout;
    CK(di.alloc(n * 12)); CK(dout.alloc(n));
    CK(hipMemcpy(di.p, rgb, n * 12, hipMemcpyHostToDevice));
    k_passes<<<blocks(n), 256>>>(*q, n, di.as<float>(), dout.as<unsigned char>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(pass, dout.p, n, hipMemcpyDeviceToHost));
    return 0;
}

int colour_probe_recolour_device(const float* a9, const float* o3, uint64_t n, const float* sh48, float* out) {
    if (n == 0) return 0;
    if (n > MAX_N || !a9 || !o3 || !sh48 || !out) return (int)hipErrorInvalidValue;
    DevBuf di, dout;
    CK(di.alloc(n * 192)); CK(dout.alloc(n * 192));
    CK(hipMemcpy(di.p, sh48, n * 192, hipMemcpyHostToDevice));
    k_recolour<<<blocks(n), 256>>>(map_of(a9, o3), n, di.as<float>(), dout.as<float>());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, n * 192, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
