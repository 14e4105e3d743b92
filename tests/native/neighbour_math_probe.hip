// neighbour_math_probe.hip -- TEST ONLY.  The predicates of the neighbourhood selection (splat_amd/csrc/splat_neighbour_math.h)
// behind C entry points, in host code, so that tests/test_neighbour_math_host.py can hold them to a numpy restatement bit
// for bit and check that the box gap never exceeds the distance of any pair of points inside the boxes.  Built by
// splat_amd/csrc/Makefile with the product's flags into tests/native/libneighbour_math_probe.so; not linked into
// libsplat_hip.so.  No GPU is needed: nothing here launches.
//
// p, q: 3 floats per row; lo_*, hi_*: 3 floats per row; the values go to d2_out / gap2_out (one float per row) and the
// verdicts against r2 = nb_radius2(radius) to within_out (one byte per row); either output may be NULL.  All host pointers.
#include <stdint.h>

#include "splat_neighbour_math.h"

extern "C" {

float neighbour_probe_radius2(float radius) { return nb_radius2(radius); }

void neighbour_probe_points(uint64_t n, const float* p, const float* q, float radius, float* d2_out, uint8_t* within_out) {
    const float r2 = nb_radius2(radius);
    for (uint64_t i = 0; i < n; ++i) {
        const float *a = p + 3 * i, *b = q + 3 * i;
        if (d2_out) d2_out[i] = nb_dist2(a[0], a[1], a[2], b[0], b[1], b[2]);
        if (within_out) within_out[i] = nb_within_reach(a[0], a[1], a[2], b[0], b[1], b[2], r2) ? 1 : 0;
    }
}

void neighbour_probe_point_box(uint64_t n, const float* lo_s, const float* hi_s, const float* p, float radius, float* gap2_out,
                               uint8_t* within_out) {
    const float r2 = nb_radius2(radius);
    for (uint64_t i = 0; i < n; ++i) {
        const float* a = p + 3 * i;
        if (gap2_out) gap2_out[i] = nb_point_gap2(lo_s + 3 * i, hi_s + 3 * i, a[0], a[1], a[2]);
        if (within_out) within_out[i] = nb_point_in_reach(lo_s + 3 * i, hi_s + 3 * i, a[0], a[1], a[2], r2) ? 1 : 0;
    }
}

void neighbour_probe_box_box(uint64_t n, const float* lo_s, const float* hi_s, const float* lo_t, const float* hi_t, float radius,
                             float* gap2_out, uint8_t* within_out) {
    const float r2 = nb_radius2(radius);
    for (uint64_t i = 0; i < n; ++i) {
        if (gap2_out) gap2_out[i] = nb_box_gap2(lo_s + 3 * i, hi_s + 3 * i, lo_t + 3 * i, hi_t + 3 * i);
        if (within_out) within_out[i] = nb_boxes_in_reach(lo_s + 3 * i, hi_s + 3 * i, lo_t + 3 * i, hi_t + 3 * i, r2) ? 1 : 0;
    }
}

}  // extern "C"
