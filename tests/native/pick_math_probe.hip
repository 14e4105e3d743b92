// pick_math_probe.hip -- TEST ONLY.  The arithmetic of the pick (splat_amd/csrc/splat_pick_math.h) behind C entry points, in
// host code, so that tests/test_pick_math_host.py can hold it to numpy and to the oracle bit for bit: the ordering key, the
// fragment and the coverage chain.  Built by splat_amd/csrc/Makefile with the product's flags into
// tests/native/libpick_math_probe.so; not linked into libsplat_hip.so.  No GPU is needed: nothing here launches.
#include <stdint.h>

#include "splat_pick_math.h"

extern "C" {

// keys_out[i] = pick_key(depth[i], index[i]); depth_back[i] = the depth the key gives back (either output may be NULL)
void pick_probe_keys(uint64_t n, const float* depth, const uint32_t* index, uint64_t* keys_out, float* depth_back) {
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t k = pick_key(depth[i], index[i]);
        if (keys_out) keys_out[i] = k;
        if (depth_back) depth_back[i] = pick_key_depth64(k);
    }
}

// alpha_out[i] = pick_fragment at sample sxy[i] of the record ra[i] = cx cy hx hy, rb[i] = A B C opacity
void pick_probe_fragment(uint64_t n, const float* sxy, const float* ra, const float* rb, int32_t y_up, float* alpha_out) {
    for (uint64_t i = 0; i < n; ++i)
        alpha_out[i] = pick_fragment(sxy[2 * i], sxy[2 * i + 1], ra[4 * i], ra[4 * i + 1], ra[4 * i + 2], ra[4 * i + 3], rb[4 * i],
                                     rb[4 * i + 1], rb[4 * i + 2], rb[4 * i + 3], y_up != 0);
}

// coverage_out[k] = the coverage after alpha[0..k] walked in this order
void pick_probe_chain(uint64_t n, const float* alpha, float* coverage_out) {
    float t = 1.0f;
    for (uint64_t k = 0; k < n; ++k) {
        t = pick_transmit(t, alpha[k]);
        coverage_out[k] = pick_coverage(t);
    }
}

}  // extern "C"
