// splat_neighbour_math.h -- the two predicates of the neighbourhood selection (splat_select_neighbours_device): whether one
// centre lies within reach of another, and whether a box -- a K1 block's resident bounds, or a single centre taken as a box
// of no extent -- can hold any centre within reach of another box.  splat_neighbours.hip includes it (the kernels), so does
// splat_scene.hip (the radius a call is refused for), and so does tests/native/neighbour_math_probe.hip, which runs it
// alone, compiled for the host (tests/test_neighbour_math_host.py).  Plain C++, __host__ __device__: one text for all.
//
// Every difference, product and sum is rounded to f32 once, in the order written -- the translation units that include
// this are compiled with -ffp-contract=off, and the formulas rest on it:
//   d2   = (dx dx + dy dy) + dz dz,   dx = p.x - q.x, dy and dz alike                     j within reach of i: d2 <= r2
//   gap2 = (g0 g0 + g1 g1) + g2 g2,   g_a = max(max(lo_s[a] - hi_t[a], lo_t[a] - hi_s[a]), 0)       the pair counts: gap2 <= r2
// A NaN fails both comparisons, and the max hands a NaN on (as numpy's maximum does, unlike fmaxf): a box with NaN bounds
// reaches nothing, a centre with a non-finite coordinate neither (its d2 is inf or NaN, and r2 is finite).
//
// The gap is a LOWER BOUND of d2, exactly and not approximately: for p inside box t and q inside box s, on every axis
// either the boxes overlap (g = 0 <= |dx|) or, say, lo_s - hi_t > 0, and then q - p >= lo_s - hi_t in the reals; f32
// subtraction rounds monotonically, so |fl(p - q)| = fl(q - p) >= fl(lo_s - hi_t) = g.  Products of non-negative floats and
// sums round monotonically too, and gap2 is evaluated in d2's order: gap2 <= d2.  So a box whose gap2 fails r2 holds no
// centre within reach, and skipping it changes no count.  No epsilon, and no box grown by r: lo - r rounds differently.
#pragma once
#include <hip/hip_runtime.h>

// radius * radius as the call uses it, rounded to f32 once
__host__ __device__ __forceinline__ float nb_radius2(float radius) { return radius * radius; }

__host__ __device__ __forceinline__ float nb_dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}
__host__ __device__ __forceinline__ bool nb_within_reach(float px, float py, float pz, float qx, float qy, float qz, float r2) {
    return nb_dist2(px, py, pz, qx, qy, qz) <= r2;
}

// the larger of two, a NaN in either handed on
__host__ __device__ __forceinline__ float nb_max(float a, float b) { return (a > b || a != a) ? a : b; }
__host__ __device__ __forceinline__ float nb_gap_axis(float lo_s, float hi_s, float lo_t, float hi_t) {
    return nb_max(nb_max(lo_s - hi_t, lo_t - hi_s), 0.0f);
}
// box s against box t (lo and hi: three floats each)
__host__ __device__ __forceinline__ float nb_box_gap2(const float* lo_s, const float* hi_s, const float* lo_t, const float* hi_t) {
    const float g0 = nb_gap_axis(lo_s[0], hi_s[0], lo_t[0], hi_t[0]);
    const float g1 = nb_gap_axis(lo_s[1], hi_s[1], lo_t[1], hi_t[1]);
    const float g2 = nb_gap_axis(lo_s[2], hi_s[2], lo_t[2], hi_t[2]);
    return (g0 * g0 + g1 * g1) + g2 * g2;
}
__host__ __device__ __forceinline__ bool nb_boxes_in_reach(const float* lo_s, const float* hi_s, const float* lo_t, const float* hi_t, float r2) {
    return nb_box_gap2(lo_s, hi_s, lo_t, hi_t) <= r2;
}
// box s against the centre p: the same expression with lo_t = hi_t = p
__host__ __device__ __forceinline__ float nb_point_gap2(const float* lo_s, const float* hi_s, float px, float py, float pz) {
    const float g0 = nb_gap_axis(lo_s[0], hi_s[0], px, px);
    const float g1 = nb_gap_axis(lo_s[1], hi_s[1], py, py);
    const float g2 = nb_gap_axis(lo_s[2], hi_s[2], pz, pz);
    return (g0 * g0 + g1 * g1) + g2 * g2;
}
__host__ __device__ __forceinline__ bool nb_point_in_reach(const float* lo_s, const float* hi_s, float px, float py, float pz, float r2) {
    return nb_point_gap2(lo_s, hi_s, px, py, pz) <= r2;
}
