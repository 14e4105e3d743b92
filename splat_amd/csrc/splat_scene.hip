// splat_scene.hip -- everything that puts values into the resident scene: the uploads (host buffers, device buffers, PLY
// rows), the in-place edits, K0 (cov3d) and the scene's layout read back -- and the selections read from it, which name the
// Gaussians such an edit is for, the removal that takes them out, the append that adds some and the reorder.  Host side only,
// no device code: the kernels are splat_kernels.hip's (order, bounds, packing), splat_ply.hip's, splat_ply_encode.hip's,
// splat_update.hip's, splat_transform.hip's, splat_select.hip's, splat_compact.hip's, splat_append.hip's,
// splat_neighbours.hip's, splat_pick.hip's, splat_colour.hip's and splat_visibility.hip's.
// What the frame scheduler (splat_api.hip) holds per scene is behind the seam of splat_context.h.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "splat_context.h"
#include "splat_colour_math.h"
#include "splat_neighbour_math.h"
#include "splat_sh_math.h"

using namespace splat;

namespace {

// helpers that return hipError_t hand a failed call's error on; the entry point's HIP_TRY names the helper and reports it
#define HIP_RET(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return _e; } while (0)

// The device buffers and events a call needs only while it runs: all of them go with their owner, on every way out.
struct Temps {
    explicit Temps(splat_ctx* ctx) : c(ctx) {}
    Temps(const Temps&) = delete;
    Temps& operator=(const Temps&) = delete;
    ~Temps() {
        for (void*& p : bufs) dfree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
    template <typename T>
    hipError_t alloc(T** p, size_t bytes) {
        hipError_t e = dmalloc(c, p, bytes);
        if (e == hipSuccess) bufs.push_back((void*)*p);
        return e;
    }
    template <typename T>
    void release(T*& p) {                      // ahead of the owner: what comes next needs the room
        bufs.erase(std::remove(bufs.begin(), bufs.end(), (void*)p), bufs.end());
        dfree(p);
    }
    template <typename T>
    T* keep(T*& p) {                           // handed on: the buffer outlives the call (a removal's new scene arrays)
        bufs.erase(std::remove(bufs.begin(), bufs.end(), (void*)p), bufs.end());
        T* q = p;
        p = nullptr;
        return q;
    }
    template <typename T>
    void adopt(T* p) {                         // made elsewhere (dmalloc), freed here
        if (p) bufs.push_back((void*)p);
    }
    hipError_t event(hipEvent_t* e) {          // (with timing)
        hipError_t err = hipEventCreate(e);
        if (err == hipSuccess) events.push_back(*e);
        return err;
    }
    splat_ctx* c;
    std::vector<void*> bufs;
    std::vector<hipEvent_t> events;
};

// A failed upload leaves no scene -- the context is as splat_upload_scene(n = 0) leaves it -- and the failure's message.
// The one exception: frames that cannot be ended (end_frames_for_upload fails) keep the scene they read, here as in an upload.
struct SceneGuard {
    splat_ctx* c;
    bool frames_ended;         // false: the old scene is still resident and its frames may be in flight (a PLY upload's decode)
    bool armed = true;         // until the upload has reached scene_installed
    ~SceneGuard() {
        if (!armed) return;
        const std::string why = c->err;
        if (frames_ended || end_frames_for_upload(c) == SPLAT_OK) free_scene(c);
        c->err = why;
    }
};

// Upload-time ordering: 30-bit Morton code of the position inside the scene's bounding box.
// order[j] = original index stored in slot j.  Ties keep index order; non-finite positions go first.
inline uint32_t spread3(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
void morton_order(uint64_t n, const float* pos4, std::vector<unsigned int>& order) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            float v = pos4[4 * i + a];
            if (std::isfinite(v)) { lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v); }
        }
    float sc[3];
    for (int a = 0; a < 3; ++a) sc[a] = (hi[a] > lo[a]) ? 1023.0f / (hi[a] - lo[a]) : 0.0f;
    std::vector<uint64_t> keyed(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t code = 0;
        for (int a = 0; a < 3; ++a) {
            float v = pos4[4 * i + a];
            uint32_t q = std::isfinite(v) ? (uint32_t)std::min(1023.0f, std::max(0.0f, (v - lo[a]) * sc[a])) : 0u;
            code |= spread3(q) << a;
        }
        keyed[i] = ((uint64_t)code << 32) | (uint64_t)i;
    }
    std::sort(keyed.begin(), keyed.end());
    order.resize(n);
    for (uint64_t j = 0; j < n; ++j) order[j] = (unsigned int)keyed[j];
}

// Bounds of every K1 block (256 consecutive slots): AABB of the finite centres, largest ||cov3d||_F.
void block_bounds(uint64_t n, const float* pos4, const float* cov3d, const std::vector<unsigned int>& order,
                  std::vector<BlockBounds>& out) {
    const uint64_t nb = (n + 255) / 256;
    out.resize(nb);
    for (uint64_t b = 0; b < nb; ++b) {
        BlockBounds bb;
        for (int a = 0; a < 3; ++a) { bb.lo[a] = INFINITY; bb.hi[a] = -INFINITY; }
        bb.fmax = 0.0f; bb.pad = 0.0f;
        const uint64_t j1 = std::min<uint64_t>(n, (b + 1) * 256);
        for (uint64_t j = b * 256; j < j1; ++j) {
            const uint64_t i = order[j];
            const float* p = pos4 + 4 * i;
            if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;   // never visible
            for (int a = 0; a < 3; ++a) { bb.lo[a] = std::min(bb.lo[a], p[a]); bb.hi[a] = std::max(bb.hi[a], p[a]); }
            double f2 = 0.0;
            for (int e = 0; e < 9; ++e) f2 += (double)cov3d[9 * i + e] * (double)cov3d[9 * i + e];
            float f = (float)std::sqrt(f2) * 1.0001f;
            if (!(f >= 0.0f)) f = INFINITY;                    // NaN: unbounded extent
            bb.fmax = std::max(bb.fmax, f);
        }
        if (!(bb.lo[0] <= bb.hi[0]))                            // no finite centre at all: NaN bounds answer "maybe"
            for (int a = 0; a < 3; ++a) { bb.lo[a] = NAN; bb.hi[a] = NAN; }
        out[b] = bb;
    }
}

// The buffers that live as long as the scene, in two parts: the frame slots' per-Gaussian buffers (a removal makes them for
// the scene it has compacted) ...
hipError_t alloc_slot_buffers(splat_ctx* c, uint64_t n) {
    for (Slot& s : c->slots) {
        HIP_RET(dmalloc(c, &s.recs, sizeof(Rec) * n));
        HIP_RET(dmalloc(c, &s.blockinfo, sizeof(unsigned int) * ((n + 255) / 256)));
        HIP_RET(hipMemsetAsync(s.blockinfo, 0, sizeof(unsigned int) * ((n + 255) / 256), c->stream));
        if (c->large_tiles >= 0) {          // (SPLAT_LARGE_TILES < 0: no list, K1's blocks expand their close-ups themselves)
            HIP_RET(dmalloc(c, &s.large_list, sizeof(uint4) * n));
            HIP_RET(dmalloc(c, &s.large_count, sizeof(unsigned int) * 4));
            HIP_RET(hipMemsetAsync(s.large_count, 0, sizeof(unsigned int) * 4, c->stream));
        }
    }
    return hipSuccess;
}
// ... and, in front of them, the scene arrays (the bounds apart: the host path makes them once it has their values)
hipError_t alloc_scene(splat_ctx* c, uint64_t n) {
    HIP_RET(dmalloc(c, &c->planes, sizeof(float4) * SCENE_PLANES * n));
    HIP_RET(dmalloc(c, &c->orig, sizeof(unsigned int) * n));
    return alloc_slot_buffers(c, n);
}
// Work the caller enqueued on `producer` comes first: the context's stream waits for an event recorded there.
hipError_t follow_producer(splat_ctx* c, void* producer) {
    if (!producer) return hipSuccess;          // (the caller has synchronised)
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    e = hipEventRecord(ev, (hipStream_t)producer);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev, 0);
    (void)hipEventDestroy(ev);                 // (released once the wait has been satisfied)
    return e;
}

// The two in-place edits (whole fields, by index) share everything but the repack and which blocks get new bounds.
constexpr uint32_t FIELDS_ALL = SPLAT_FIELD_POS | SPLAT_FIELD_COV3D | SPLAT_FIELD_OPACITY | SPLAT_FIELD_SH;
// what both refuse before they touch HIP (rows: n or k); nullptr: nothing
const char* update_refusal(uint64_t rows, uint32_t fields, const void* pos4, const void* cov3d, const void* opacity, const void* sh) {
    if (fields & ~FIELDS_ALL) return "unknown bits in fields";
    if (rows && (((fields & SPLAT_FIELD_POS) && !pos4) || ((fields & SPLAT_FIELD_COV3D) && !cov3d) ||
                 ((fields & SPLAT_FIELD_OPACITY) && !opacity) || ((fields & SPLAT_FIELD_SH) && !sh)))
        return "NULL pointer for a named field";
    return nullptr;
}
// the inverse of the scene's order, the index check's counter and the dirty bytes: made by the first indexed edit of a scene
hipError_t ensure_inverse(splat_ctx* c) {
    if (c->inv) return hipSuccess;
    const uint64_t n = c->n, nb = (n + 255) / 256;
    HIP_RET(dmalloc(c, &c->inv, sizeof(unsigned int) * n + 16 + nb));
    c->upd_bad = c->inv + n;
    c->upd_dirty = (unsigned char*)(c->inv + n) + 16;
    hipError_t e = hipMemsetAsync(c->upd_bad, 0, 16 + nb, c->stream);
    if (e != hipSuccess) { dfree(c->inv); c->upd_bad = nullptr; c->upd_dirty = nullptr; return e; }
    launch_inverse_order(c->stream, n, c->orig, c->inv);
    return hipGetLastError();
}

// the indices of an indexed edit or read: how many name no Gaussian comes back before anything is written (after ensure_inverse)
hipError_t count_bad_indices(splat_ctx* c, uint64_t k, const unsigned int* index, unsigned int* bad) {
    HIP_RET(hipMemsetAsync(c->upd_bad, 0, sizeof(unsigned int), c->stream));
    launch_index_check(c->stream, k, c->n, index, c->upd_bad);
    HIP_RET(hipGetLastError());
    HIP_RET(hipMemcpyAsync(bad, c->upd_bad, sizeof *bad, hipMemcpyDeviceToHost, c->stream));
    return hipStreamSynchronize(c->stream);
}

// the camera (nullable) and the context's conventions as the scene queries' kernels take them; W and H are the caller's to set
SelectView select_view(const splat_ctx* c, const splat_camera* cam) {
    SelectView v{};
    if (cam) {
        std::copy(cam->view, cam->view + 16, v.view);
        std::copy(cam->proj, cam->proj + 16, v.proj);
        v.w = cam->w; v.h = cam->h; v.htanx = cam->htanx; v.htany = cam->htany; v.focal = cam->focal; v.lowpass = cam->lowpass;
    }
    v.y_up = c->cfg.y_up; v.sample_half = c->cfg.sample_half; v.zclip = c->cfg.zclip; v.zmin = c->cfg.zmin; v.zmax = c->cfg.zmax;
    v.corrected = (c->cfg.mode & SPLAT_MODE_CORRECTED_PROJECTION) ? 1 : 0;
    return v;
}

// what splat_select_device refuses before it looks at the context or touches HIP; nullptr: nothing
constexpr uint32_t SEL_TESTS_ALL = SPLAT_SEL_VOLUME | SPLAT_SEL_SCREEN | SPLAT_SEL_DEPTH | SPLAT_SEL_OPACITY;
const char* select_refusal(const splat_select_query* q, const splat_camera* cam, const void* pixel_mask, uint32_t op) {
    if (!q) return "NULL query";
    if (q->tests & ~SEL_TESTS_ALL) return "unknown bits in tests";
    if (op > SPLAT_SEL_OP_INTERSECT) return "unknown op";
    if (q->volume_shape > 1u) return "unknown volume_shape";
    if (q->screen_rule > 1u) return "unknown screen_rule";
    if ((q->tests & (SPLAT_SEL_SCREEN | SPLAT_SEL_DEPTH)) && !cam) return "SCREEN or DEPTH named without a camera";
    if ((q->tests & SPLAT_SEL_SCREEN) && (!(cam->w >= 1.0f) || !(cam->h >= 1.0f) || cam->w > 65535.0f || cam->h > 65535.0f ||
                                          cam->w != std::floor(cam->w) || cam->h != std::floor(cam->h)))
        return "camera w/h must be integers in [1, 65535]";
    if ((q->tests & SPLAT_SEL_SCREEN) && q->screen_rule == 1u && pixel_mask) return "a pixel mask goes with the centre rule, not with touch";
    return nullptr;
}

// what splat_select_neighbours_device refuses before it looks at the context or touches HIP; nullptr: nothing
const char* neighbours_refusal(float radius, uint32_t count_min, uint32_t count_max, uint32_t op, const void* selection,
                               const void* counts_out) {
    if (!(radius >= 0.0f)) return "radius is NaN or negative";
    if (!std::isfinite(nb_radius2(radius))) return "radius: radius * radius is not finite in f32";
    if (count_min > count_max) return "count_min is above count_max";
    if (op > SPLAT_SEL_OP_INTERSECT) return "unknown op";
    if (!selection && !counts_out) return "d_selection and d_counts_out are both NULL";
    if ((uintptr_t)counts_out & 3u) return "d_counts_out is misaligned (4 bytes)";
    return nullptr;
}

// what splat_pick_device refuses before it looks at the context or touches HIP; nullptr: nothing
const char* pick_refusal(const splat_pick_query* q, const splat_camera* cam, uint32_t n_pixels, const int32_t* pixels_xy,
                         const void* results, const void* layers) {
    if (!q) return "NULL q";
    if (!cam) return "NULL cam";
    if (!(cam->w >= 1.0f) || !(cam->h >= 1.0f) || cam->w > 65535.0f || cam->h > 65535.0f || cam->w != std::floor(cam->w) ||
        cam->h != std::floor(cam->h))
        return "cam: w/h must be integers in [1, 65535]";
    if (n_pixels > SPLAT_PICK_MAX_PIXELS) return "n_pixels is above SPLAT_PICK_MAX_PIXELS (256)";
    if (q->max_hits < 1u || q->max_hits > SPLAT_PICK_MAX_HITS) return "max_hits is outside [1, SPLAT_PICK_MAX_HITS (4096)]";
    if (q->max_layers > q->max_hits) return "max_layers is above max_hits";
    if (!(q->coverage_min > 0.0f) || !(q->coverage_min <= 1.0f)) return "coverage_min is not in (0, 1]";
    if (q->alpha_min != q->alpha_min) return "alpha_min is NaN";
    if (q->max_layers > 0u && !layers) return "NULL d_layers with max_layers > 0";
    if (((uintptr_t)results | (uintptr_t)layers) & 3u) return "d_results or d_layers is misaligned (4 bytes)";
    if (n_pixels && !pixels_xy) return "NULL pixels_xy";
    if (n_pixels && !results) return "NULL d_results";
    const int W = (int)cam->w, H = (int)cam->h;
    for (uint32_t p = 0; p < n_pixels; ++p)
        if (pixels_xy[2 * p] < 0 || pixels_xy[2 * p] >= W || pixels_xy[2 * p + 1] < 0 || pixels_xy[2 * p + 1] >= H)
            return "pixels_xy: a pixel lies outside [0, w) x [0, h)";
    return nullptr;
}

// what splat_visibility_device and splat_select_counts_device refuse before they look at the context or touch HIP; nullptr: nothing
const char* visibility_refusal(const splat_visibility_query* q, const splat_camera* cam, const void* pixels, const void* max_weight,
                               const void* weight_sum) {
    if (!q) return "NULL q";
    if (!cam) return "NULL cam";
    if (!(q->weight_min >= 0.0f) || !(q->weight_min < 1.0f)) return "q: weight_min is not in [0, 1)";
    if (q->op > SPLAT_VIS_ACCUMULATE) return "q: unknown op";
    if (!(cam->w >= 1.0f) || !(cam->h >= 1.0f) || cam->w > 65535.0f || cam->h > 65535.0f || cam->w != std::floor(cam->w) ||
        cam->h != std::floor(cam->h))
        return "cam: w/h must be integers in [1, 65535]";
    if ((uintptr_t)pixels & 3u) return "d_pixels is misaligned (4 bytes)";
    if ((uintptr_t)max_weight & 3u) return "d_max_weight is misaligned (4 bytes)";
    if ((uintptr_t)weight_sum & 7u) return "d_weight_sum is misaligned (8 bytes)";
    if (!pixels && !max_weight && !weight_sum) return "d_pixels, d_max_weight and d_weight_sum are all NULL";
    return nullptr;
}
const char* select_counts_refusal(uint64_t n, const void* counts, uint32_t count_min, uint32_t count_max, uint32_t op, const void* selection) {
    if (count_min > count_max) return "count_min is above count_max";
    if (op > SPLAT_SEL_OP_INTERSECT) return "unknown op";
    if (n >= (1ull << 32)) return "n: too many counts (an index is 32-bit)";
    if (n && !counts) return "NULL d_counts";
    if ((uintptr_t)counts & 3u) return "d_counts is misaligned (4 bytes)";
    if (n && !selection) return "NULL d_selection";
    return nullptr;
}

// what the two colour queries refuse before they look at the context or touch HIP; nullptr: nothing
const char* eval_colours_refusal(const splat_camera* cam, uint64_t k, const void* rgb_out) {
    if (!cam) return "NULL cam";
    if (k && !rgb_out) return "NULL d_rgb_out";
    if (k && ((uintptr_t)rgb_out & 3u)) return "d_rgb_out is misaligned (4 bytes)";
    return nullptr;
}
const char* select_colour_refusal(const splat_colour_query* q, const splat_camera* cam, uint32_t op, const void* selection) {
    if (!q) return "NULL q";
    if (!cam) return "NULL cam";
    if (q->shape > 1u) return "q: unknown shape";
    if (op > SPLAT_SEL_OP_INTERSECT) return "unknown op";
    if (!selection) return "NULL d_selection";
    return nullptr;
}

// what splat_remove_gaussians_device refuses before it looks at the context or touches HIP; nullptr: nothing
const char* remove_refusal(uint64_t n, const void* selection, uint32_t mode, const void* index_map, const uint64_t* n_out) {
    if (!n_out) return "NULL n_out";
    if (mode > SPLAT_REMOVE_UNSELECTED) return "unknown mode";
    if ((uintptr_t)index_map & 3u) return "d_index_map_out is misaligned (4 bytes)";
    if (n && !selection) return "NULL d_selection";
    return nullptr;
}

// what splat_append_gaussians_device refuses before it looks at the context or touches HIP; nullptr: nothing
const char* append_refusal(uint64_t n, uint64_t m, const void* pos4, const void* cov3d, const void* opacity, const void* sh,
                           const uint64_t* n_out) {
    if (!n_out) return "NULL n_out";
    if (n >= 0xFFFFFFFFull || m >= 0xFFFFFFFFull - n) return "n + m: too many Gaussians (an index is 32-bit)";
    if (m && !pos4) return "NULL d_pos4";
    if (m && !cov3d) return "NULL d_cov3d";
    if (m && !opacity) return "NULL d_opacity";
    if (m && !sh) return "NULL d_sh";
    return nullptr;
}

// what both PLY entry points refuse before they touch HIP; msg: why
bool ply_layout_ok(const splat_ply_layout* lay, const char** msg) {
    if (!lay) { *msg = "NULL layout"; return false; }
    if (lay->stride == 0) { *msg = "PLY stride is 0"; return false; }
    for (int k = 0; k < SPLAT_PLY_SLOTS; ++k) {
        if (lay->offset[k] < -1) { *msg = "PLY property offset below -1"; return false; }
        if (lay->offset[k] >= 0 && (uint64_t)lay->offset[k] + 4u > lay->stride) { *msg = "PLY property reaches beyond its row"; return false; }
    }
    if (lay->n >= 0xFFFFFFFFull) { *msg = "too many Gaussians (index is 32-bit)"; return false; }
    return true;
}
// decode + recentre on the context's stream, behind `producer`, waited for; the mean's three floats are the chain's only
// temporary.
hipError_t ply_decode_now(splat_ctx* c, const splat_ply_layout& lay, const void* d_rows, float* pos4, float* scales3,
                          float* opacity, float* rot4, float* sh, void* producer) {
    Temps t(c);
    float* d_mean = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    HIP_RET(t.alloc(&d_mean, sizeof(float) * 4));
    for (hipEvent_t& x : ev) HIP_RET(t.event(&x));
    HIP_RET(follow_producer(c, producer));
    launch_ply_decode(c->stream, lay, d_rows, pos4, scales3, opacity, rot4, sh, d_mean, ev);
    HIP_RET(hipGetLastError());
    HIP_RET(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; ++k) { c->ply_ms[k] = 0.0f; (void)hipEventElapsedTime(&c->ply_ms[k], ev[k], ev[k + 1]); }
    return hipSuccess;
}

// what both PLY encoders refuse before they look at the context or touch HIP (rows: the resident n is judged later, k here);
// nullptr: nothing.  The kernel owns whole dwords: everything that places a float is a multiple of 4.
const char* ply_encode_refusal(const splat_ply_layout* lay, const void* d_rows) {
    if (!lay) return "NULL layout";
    if ((uintptr_t)d_rows & 3u) return "d_rows_out is misaligned (4 bytes)";
    if (lay->stride == 0) return "layout->stride is 0";
    if (lay->stride & 3u) return "layout->stride is not a multiple of 4";
    if (lay->stride > PLY_STAGE_BYTES) return "layout->stride is above 65528 bytes: a row must fit the encoder's stage";
    if (lay->n >= 0xFFFFFFFFull) return "layout->n: too many rows (an index is 32-bit)";
    int present[SPLAT_PLY_SLOTS], m = 0;
    for (int k = 0; k < SPLAT_PLY_SLOTS; ++k) {
        const int32_t o = lay->offset[k];
        if (o < -1) return "layout->offset below -1";
        if (o < 0) continue;
        if (o & 3) return "layout->offset is not a multiple of 4";
        if ((uint64_t)o + 4u > lay->stride) return "layout->offset reaches beyond layout->stride";
        present[m++] = o;
    }
    std::sort(present, present + m);
    for (int k = 1; k < m; ++k)
        if (present[k] == present[k - 1]) return "layout->offset: two present properties overlap";
    if (lay->n && !d_rows) return "NULL d_rows_out";
    const uint64_t rows = std::min<uint64_t>(PLY_ROWS, PLY_STAGE_BYTES / lay->stride);
    if ((lay->n + rows - 1) / rows > 0x7FFFFFFFull) return "layout->n: more workgroups than one launch holds";
    return nullptr;
}
}  // namespace

namespace splat {
void free_scene(splat_ctx* c) {
    dfree(c->planes); dfree(c->orig); dfree(c->bounds);
    dfree(c->inv); c->upd_bad = nullptr; c->upd_dirty = nullptr;
    for (Slot& s : c->slots) { dfree(s.recs); dfree(s.depth); dfree(s.rect); dfree(s.vislist); dfree(s.blockinfo); dfree(s.large_list); dfree(s.large_count); s.used = false; }
    c->n = 0;
    c->h_orig.clear();
    c->last_slot = -1;
}
// The host copy of the scene's order (the debug getters translate slots with it): the host upload leaves it behind, a
// device upload does not -- it is fetched when first asked for.
int ensure_h_orig(splat_ctx* c) {
    if (c->h_orig.size() == c->n) return SPLAT_OK;
    std::vector<unsigned int> h(c->n);
    if (c->n) HIP_TRY(c, hipMemcpy(h.data(), c->orig, sizeof(unsigned int) * c->n, hipMemcpyDeviceToHost));
    c->h_orig.swap(h);
    return SPLAT_OK;
}
}  // namespace splat

extern "C" {

// The two scene uploads (host buffers, device buffers) share everything but how the order, the bounds and the planes get
// their values: the frames of the scene being replaced end, the old scene goes, the new one is made and installed.  Their
// temporaries go before scene_installed makes the key buffers: the upload's peak is the scene's own.
int splat_upload_scene(splat_ctx* c, uint64_t n, const float* pos4, const float* cov3d, const float* opacity,
                       const float* sh) {
    if (!c) return SPLAT_ERR_INVALID;
    if (n && (!pos4 || !cov3d || !opacity || !sh)) return fail(c, SPLAT_ERR_INVALID, "NULL scene pointer");
    if (n >= 0xFFFFFFFFull) return fail(c, SPLAT_ERR_INVALID, "too many Gaussians (index is 32-bit)");
    int rc = end_frames_for_upload(c);
    if (rc != SPLAT_OK) return rc;
    free_scene(c);
    if (n == 0) return SPLAT_OK;
    SceneGuard guard{c, true};
    morton_order(n, pos4, c->h_orig);
    {
        Temps t(c);
        float *d_pos = nullptr, *d_cov = nullptr, *d_op = nullptr, *d_sh = nullptr;
        HIP_TRY(c, alloc_scene(c, n));
        HIP_TRY(c, hipMemcpyAsync(c->orig, c->h_orig.data(), sizeof(unsigned int) * n, hipMemcpyHostToDevice, c->stream));
        std::vector<BlockBounds> hb;
        block_bounds(n, pos4, cov3d, c->h_orig, hb);
        HIP_TRY(c, dmalloc(c, &c->bounds, sizeof(BlockBounds) * hb.size()));
        HIP_TRY(c, hipMemcpyAsync(c->bounds, hb.data(), sizeof(BlockBounds) * hb.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, t.alloc(&d_pos, sizeof(float) * 4 * n));
        HIP_TRY(c, t.alloc(&d_cov, sizeof(float) * 9 * n));
        HIP_TRY(c, t.alloc(&d_op, sizeof(float) * n));
        HIP_TRY(c, t.alloc(&d_sh, sizeof(float) * 48 * n));
        HIP_TRY(c, hipMemcpyAsync(d_pos, pos4, sizeof(float) * 4 * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_cov, cov3d, sizeof(float) * 9 * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_op, opacity, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_sh, sh, sizeof(float) * 48 * n, hipMemcpyHostToDevice, c->stream));
        launch_pack_scene(c->stream, n, d_pos, d_cov, d_op, d_sh, c->orig, c->planes);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    scene_installed(c, n);
    guard.armed = false;
    return SPLAT_OK;
}

int splat_upload_scene_device(splat_ctx* c, uint64_t n, const void* d_pos4, const void* d_cov3d, const void* d_opacity,
                              const void* d_sh, void* producer_stream) {
    if (!c) return SPLAT_ERR_INVALID;
    if (n && (!d_pos4 || !d_cov3d || !d_opacity || !d_sh)) return fail(c, SPLAT_ERR_INVALID, "NULL scene pointer");
    if (n >= 0xFFFFFFFFull) return fail(c, SPLAT_ERR_INVALID, "too many Gaussians (index is 32-bit)");
    int rc = end_frames_for_upload(c);
    if (rc != SPLAT_OK) return rc;
    free_scene(c);
    if (n == 0) return SPLAT_OK;
    SceneGuard guard{c, true};
    const float *pos4 = (const float*)d_pos4, *cov3d = (const float*)d_cov3d;
    {
        // the sort's ping-pong arrays (16 B per Gaussian) and its scan tables: all that exists beside the scene itself
        Temps t(c);
        uint32_t* d_sort = nullptr; unsigned char* d_small = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        HIP_TRY(c, alloc_scene(c, n));
        HIP_TRY(c, dmalloc(c, &c->bounds, sizeof(BlockBounds) * ((n + 255) / 256)));
        HIP_TRY(c, t.alloc(&d_sort, sizeof(uint32_t) * 4 * n));
        HIP_TRY(c, t.alloc(&d_small, scene_order_small_bytes(n)));
        HIP_TRY(c, t.event(&ev[0]));
        HIP_TRY(c, t.event(&ev[1]));
        HIP_TRY(c, follow_producer(c, producer_stream));
        launch_scene_order(c->stream, n, pos4, d_sort, d_small, c->orig, ev[0], ev[1]);
        launch_block_bounds(c->stream, n, pos4, cov3d, c->orig, c->bounds);
        launch_pack_scene(c->stream, n, pos4, cov3d, (const float*)d_opacity, (const float*)d_sh, c->orig, c->planes);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->upload_sort_ms = 0.0f;
        (void)hipEventElapsedTime(&c->upload_sort_ms, ev[0], ev[1]);
    }
    scene_installed(c, n);
    guard.armed = false;
    return SPLAT_OK;
}

// (debug, not part of the ABI)  Device time of the sort inside the most recent splat_upload_scene_device, in milliseconds.
int splat_debug_upload_sort_ms(splat_ctx* c, double* ms) {
    if (!c || !ms) return SPLAT_ERR_INVALID;
    *ms = c->upload_sort_ms;
    return SPLAT_OK;
}

int splat_update_scene_device(splat_ctx* c, uint64_t n, uint32_t fields, const void* d_pos4, const void* d_cov3d,
                              const void* d_opacity, const void* d_sh, void* producer_stream) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (const char* why = update_refusal(n, fields, d_pos4, d_cov3d, d_opacity, d_sh)) return fail(c, SPLAT_ERR_INVALID, why);
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to update");
    if (n != c->n) return fail(c, SPLAT_ERR_INVALID, "n is not the resident scene's (changing n is an upload or a removal)");
    if (fields == 0) return SPLAT_OK;
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_repack_scene(c->stream, n, fields, (const float*)d_pos4, (const float*)d_cov3d, (const float*)d_opacity, (const float*)d_sh,
                        c->orig, c->planes);
    if (fields & (SPLAT_FIELD_POS | SPLAT_FIELD_COV3D)) launch_plane_bounds(c->stream, n, c->planes, nullptr, c->bounds);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

int splat_update_gaussians_device(splat_ctx* c, uint64_t k, const void* d_index, uint32_t fields, const void* d_pos4,
                                  const void* d_cov3d, const void* d_opacity, const void* d_sh, void* producer_stream) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (const char* why = update_refusal(k, fields, d_pos4, d_cov3d, d_opacity, d_sh)) return fail(c, SPLAT_ERR_INVALID, why);
    if (k && !d_index) return fail(c, SPLAT_ERR_INVALID, "NULL index");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to update");
    if (k > c->n) return fail(c, SPLAT_ERR_INVALID, "more indices than Gaussians: they cannot be distinct");
    if (fields == 0 || k == 0) return SPLAT_OK;
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    const uint64_t n = c->n;
    const unsigned int* index = (const unsigned int*)d_index;
    HIP_TRY(c, ensure_inverse(c));
    HIP_TRY(c, follow_producer(c, producer_stream));
    // the indices first: the count of those that name no Gaussian comes back before anything is written
    unsigned int bad = 0;
    HIP_TRY(c, count_bad_indices(c, k, index, &bad));
    if (bad) return fail(c, SPLAT_ERR_INVALID, "an index is not below n; nothing was applied");
    const bool rebound = (fields & (SPLAT_FIELD_POS | SPLAT_FIELD_COV3D)) != 0;
    launch_repack_indexed(c->stream, n, k, index, fields, (const float*)d_pos4, (const float*)d_cov3d, (const float*)d_opacity,
                          (const float*)d_sh, c->inv, c->planes, rebound ? c->upd_dirty : nullptr);
    if (rebound) launch_plane_bounds(c->stream, n, c->planes, c->upd_dirty, c->bounds);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

// The inverses of the two edits: the named fields of the resident scene into the caller's device buffers.  They READ the
// scene as a selection does -- behind the frames in flight, nothing of a frame's state touched -- and refuse what the edits
// refuse (update_refusal).
int splat_read_scene_device(splat_ctx* c, uint64_t n, uint32_t fields, void* d_pos4, void* d_cov3d, void* d_opacity, void* d_sh) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (const char* why = update_refusal(n, fields, d_pos4, d_cov3d, d_opacity, d_sh)) return fail(c, SPLAT_ERR_INVALID, why);
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to read");
    if (n != c->n) return fail(c, SPLAT_ERR_INVALID, "n is not the resident scene's");
    if (fields == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    launch_unpack_scene(c->stream, n, fields, (float*)d_pos4, (float*)d_cov3d, (float*)d_opacity, (float*)d_sh, c->orig, c->planes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

int splat_read_gaussians_device(splat_ctx* c, uint64_t k, const void* d_index, uint32_t fields, void* d_pos4, void* d_cov3d,
                                void* d_opacity, void* d_sh, void* producer_stream) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (const char* why = update_refusal(k, fields, d_pos4, d_cov3d, d_opacity, d_sh)) return fail(c, SPLAT_ERR_INVALID, why);
    if (k && !d_index) return fail(c, SPLAT_ERR_INVALID, "NULL index");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to read");
    if (k > c->n) return fail(c, SPLAT_ERR_INVALID, "more indices than Gaussians: the rows could not go back as an update");
    if (fields == 0 || k == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    const unsigned int* index = (const unsigned int*)d_index;
    HIP_TRY(c, ensure_inverse(c));
    HIP_TRY(c, follow_producer(c, producer_stream));
    unsigned int bad = 0;
    HIP_TRY(c, count_bad_indices(c, k, index, &bad));
    if (bad) return fail(c, SPLAT_ERR_INVALID, "an index is not below n; nothing was written");
    launch_unpack_indexed(c->stream, c->n, k, index, fields, (float*)d_pos4, (float*)d_cov3d, (float*)d_opacity, (float*)d_sh, c->inv,
                          c->planes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

// An affine map applied where the values lie: an edit like the two above it, with nothing taken from the caller but the
// twelve floats.  Positions and covariances change, so the bounds are always made again.
int splat_transform_scene_device(splat_ctx* c, const float m[12]) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (!m) return fail(c, SPLAT_ERR_INVALID, "NULL matrix");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to transform");
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    launch_transform_scene(c->stream, c->n, m, c->planes);
    launch_plane_bounds(c->stream, c->n, c->planes, nullptr, c->bounds);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

int splat_transform_gaussians_device(splat_ctx* c, uint64_t k, const void* d_index, const float m[12], void* producer_stream) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (!m) return fail(c, SPLAT_ERR_INVALID, "NULL matrix");
    if (k && !d_index) return fail(c, SPLAT_ERR_INVALID, "NULL index");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to transform");
    if (k > c->n) return fail(c, SPLAT_ERR_INVALID, "more indices than Gaussians: they cannot be distinct");
    if (k == 0) return SPLAT_OK;
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    const unsigned int* index = (const unsigned int*)d_index;
    HIP_TRY(c, ensure_inverse(c));
    HIP_TRY(c, follow_producer(c, producer_stream));
    unsigned int bad = 0;
    HIP_TRY(c, count_bad_indices(c, k, index, &bad));
    if (bad) return fail(c, SPLAT_ERR_INVALID, "an index is not below n; nothing was applied");
    launch_transform_indexed(c->stream, c->n, k, index, m, c->inv, c->planes, c->upd_dirty);
    launch_plane_bounds(c->stream, c->n, c->planes, c->upd_dirty, c->bounds);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

// View-dependent colour turned with the scene: the sh counterpart of the transforms.  The blocks are made on the host
// (splat_sh_math.h) from an r that has passed the orthogonality check; the device calls are edits of sh alone, so the
// bounds stay.
int splat_sh_rotation_blocks(const float r[9], float d1[9], float d2[25], float d3[49]) {
    if (!r || !d1 || !d2 || !d3) return fail(nullptr, SPLAT_ERR_INVALID, "NULL pointer");
    if (const char* why = sh_rotation_refusal(r)) return fail(nullptr, SPLAT_ERR_INVALID, why);
    SplatShBlocks b;
    sh_rotation_blocks(r, b);
    std::copy(b.d1, b.d1 + 9, d1);
    std::copy(b.d2, b.d2 + 25, d2);
    std::copy(b.d3, b.d3 + 49, d3);
    return SPLAT_OK;
}

int splat_rotate_sh_scene_device(splat_ctx* c, const float r[9]) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (!r) return fail(c, SPLAT_ERR_INVALID, "NULL matrix");
    if (const char* why = sh_rotation_refusal(r)) return fail(c, SPLAT_ERR_INVALID, why);
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to rotate");
    SplatShBlocks b;
    sh_rotation_blocks(r, b);
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    launch_rotate_sh_scene(c->stream, c->n, b, c->planes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

int splat_rotate_sh_gaussians_device(splat_ctx* c, uint64_t k, const void* d_index, const float r[9], void* producer_stream) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (!r) return fail(c, SPLAT_ERR_INVALID, "NULL matrix");
    if (const char* why = sh_rotation_refusal(r)) return fail(c, SPLAT_ERR_INVALID, why);
    if (k && !d_index) return fail(c, SPLAT_ERR_INVALID, "NULL index");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to rotate");
    if (k > c->n) return fail(c, SPLAT_ERR_INVALID, "more indices than Gaussians: they cannot be distinct");
    if (k == 0) return SPLAT_OK;
    SplatShBlocks b;
    sh_rotation_blocks(r, b);
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    const unsigned int* index = (const unsigned int*)d_index;
    HIP_TRY(c, ensure_inverse(c));
    HIP_TRY(c, follow_producer(c, producer_stream));
    unsigned int bad = 0;
    HIP_TRY(c, count_bad_indices(c, k, index, &bad));
    if (bad) return fail(c, SPLAT_ERR_INVALID, "an index is not below n; nothing was applied");
    launch_rotate_sh_indexed(c->stream, c->n, k, index, b, c->inv, c->planes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

// Colour.  The two queries READ the scene as the selection below does; the two recolours are edits of sh alone, like the
// rotations above: the map is made on the host (splat_colour_math.h) from an m whose entries and offset are finite, and the
// bounds stay.  Arguments first, then the context, then what needs the scene's n.
int splat_eval_colours_device(splat_ctx* c, const splat_camera* cam, uint64_t k, const void* d_index, void* d_rgb_out,
                              void* producer_stream) {
    if (const char* why = eval_colours_refusal(cam, k, d_rgb_out)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to evaluate");
    if (k > c->n) return fail(c, SPLAT_ERR_INVALID, "k: more rows than Gaussians");
    if (!d_index && k != c->n) return fail(c, SPLAT_ERR_INVALID, "k is not the resident scene's n (NULL d_index: all Gaussians)");
    if (k == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    if (!d_index) {
        launch_eval_colours_scene(c->stream, c->n, cam->cam_pos, cam->sh_dim, c->orig, c->planes, (float*)d_rgb_out);
    } else {
        const unsigned int* index = (const unsigned int*)d_index;
        HIP_TRY(c, ensure_inverse(c));
        HIP_TRY(c, follow_producer(c, producer_stream));
        unsigned int bad = 0;
        HIP_TRY(c, count_bad_indices(c, k, index, &bad));
        if (bad) return fail(c, SPLAT_ERR_INVALID, "d_index: an index is not below n; nothing was written");
        launch_eval_colours_indexed(c->stream, c->n, k, index, cam->cam_pos, cam->sh_dim, c->inv, c->planes, (float*)d_rgb_out);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

int splat_select_colour_device(splat_ctx* c, const splat_colour_query* q, const splat_camera* cam, uint32_t op, void* d_selection,
                               uint64_t* count_out, void* producer_stream) {
    if (const char* why = select_colour_refusal(q, cam, op, d_selection)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to select from");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    Temps t(c);
    unsigned int* d_count = nullptr;
    unsigned int count = 0;
    HIP_TRY(c, t.alloc(&d_count, sizeof(unsigned int)));
    HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(unsigned int), c->stream));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_select_colour(c->stream, c->n, c->planes, c->orig, *q, cam->cam_pos, cam->sh_dim, op, (unsigned char*)d_selection, d_count);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (count_out) *count_out = count;
    return SPLAT_OK;
}

int splat_recolour_scene_device(splat_ctx* c, const float m[12]) {
    if (!m) return fail(c, SPLAT_ERR_INVALID, "NULL m");
    SplatColourMap map;
    if (const char* why = recolour_map(m, map)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to recolour");
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    launch_recolour_scene(c->stream, c->n, map, c->planes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

int splat_recolour_gaussians_device(splat_ctx* c, uint64_t k, const void* d_index, const float m[12], void* producer_stream) {
    if (!m) return fail(c, SPLAT_ERR_INVALID, "NULL m");
    SplatColourMap map;
    if (const char* why = recolour_map(m, map)) return fail(c, SPLAT_ERR_INVALID, why);
    if (k && !d_index) return fail(c, SPLAT_ERR_INVALID, "NULL d_index");
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to recolour");
    if (k > c->n) return fail(c, SPLAT_ERR_INVALID, "k: more indices than Gaussians: they cannot be distinct");
    if (k == 0) return SPLAT_OK;
    int rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    const unsigned int* index = (const unsigned int*)d_index;
    HIP_TRY(c, ensure_inverse(c));
    HIP_TRY(c, follow_producer(c, producer_stream));
    unsigned int bad = 0;
    HIP_TRY(c, count_bad_indices(c, k, index, &bad));
    if (bad) return fail(c, SPLAT_ERR_INVALID, "d_index: an index is not below n; nothing was applied");
    launch_recolour_indexed(c->stream, c->n, k, index, map, c->inv, c->planes);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scene_edited(c);
    return SPLAT_OK;
}

// The selection reads the scene as K1 does -- whole target, the context's conventions and mode -- and nothing of a frame's
// state: no slot, no hint, no policy is touched, and what it allocates goes with the call.
int splat_select_device(splat_ctx* c, const splat_select_query* q, const splat_camera* cam, const void* d_pixel_mask, uint32_t op,
                        void* d_selection, uint64_t* count_out, void* producer_stream) {
    // (the arguments are judged before the context is looked at, as the PLY entry points do it)
    if (const char* why = select_refusal(q, cam, d_pixel_mask, op)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to select from");
    if (!d_selection) return fail(c, SPLAT_ERR_INVALID, "NULL selection");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    splat_select_query k = *q;
    SelectView v = select_view(c, cam);
    if (k.tests & SPLAT_SEL_SCREEN) {
        v.W = (int)cam->w; v.H = (int)cam->h;
        k.x0 = std::max(k.x0, 0); k.y0 = std::max(k.y0, 0);
        k.x1 = std::min(k.x1, v.W - 1); k.y1 = std::min(k.y1, v.H - 1);
    }
    Temps t(c);
    unsigned int* d_count = nullptr;
    unsigned int count = 0;
    HIP_TRY(c, t.alloc(&d_count, sizeof(unsigned int)));
    HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(unsigned int), c->stream));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_select_query(c->stream, c->n, c->planes, c->orig, k, v, (k.tests & SPLAT_SEL_SCREEN) ? (const unsigned char*)d_pixel_mask : nullptr,
                        op, (unsigned char*)d_selection, d_count);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (count_out) *count_out = count;
    return SPLAT_OK;
}

int splat_selection_indices_device(splat_ctx* c, uint64_t n, const void* d_selection, void* d_index_out, uint64_t capacity,
                                   uint64_t* count_out, void* producer_stream) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (!count_out) return fail(c, SPLAT_ERR_INVALID, "NULL count_out");
    if (n >= (1ull << 32)) return fail(c, SPLAT_ERR_INVALID, "too many bytes in the selection (an index is 32-bit)");
    if (n && !d_selection) return fail(c, SPLAT_ERR_INVALID, "NULL selection");
    if (n && capacity && (!d_index_out || ((uintptr_t)d_index_out & 3u))) return fail(c, SPLAT_ERR_INVALID, "NULL or misaligned index buffer");
    *count_out = 0;
    if (n == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    Temps t(c);
    unsigned int* d_counts = nullptr;
    unsigned int count = 0;
    const uint64_t g = selection_groups(d_selection, n);
    HIP_TRY(c, t.alloc(&d_counts, sizeof(unsigned int) * (g + 1)));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_selection_indices(c->stream, n, (const unsigned char*)d_selection, (unsigned int*)d_index_out, capacity, d_counts);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&count, d_counts + g, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *count_out = count;
    return SPLAT_OK;
}

// The selection by neighbourhood reads the scene as the one above does.  The work bound comes back first: nothing of the
// caller's is written before the block pairs are known to be within max_block_pairs.
int splat_select_neighbours_device(splat_ctx* c, float radius, const void* d_source, uint32_t count_min, uint32_t count_max, uint32_t op,
                                   void* d_selection, void* d_counts_out, uint64_t max_block_pairs, uint64_t* block_pairs_out,
                                   uint64_t* count_out, void* producer_stream) {
    if (const char* why = neighbours_refusal(radius, count_min, count_max, op, d_selection, d_counts_out)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to select from");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    const uint64_t n = c->n;
    const float r2 = nb_radius2(radius);
    const unsigned int cap = count_max < 0xFFFFFFFFu ? count_max + 1u : 0xFFFFFFFFu;
    Temps t(c);
    unsigned long long* d_pairs = nullptr;     // the block pairs, and behind them the count of what is selected
    unsigned int* d_counts = (unsigned int*)d_counts_out;
    unsigned long long pairs = 0;
    unsigned int count = 0;
    HIP_TRY(c, t.alloc(&d_pairs, 2 * sizeof(unsigned long long)));
    unsigned int* const d_count = (unsigned int*)(d_pairs + 1);
    HIP_TRY(c, hipMemsetAsync(d_pairs, 0, 2 * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_neighbour_block_pairs(c->stream, n, c->bounds, r2, d_pairs);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&pairs, d_pairs, sizeof pairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (block_pairs_out) *block_pairs_out = pairs;
    if (max_block_pairs != 0 && pairs > max_block_pairs)
        return fail(c, SPLAT_ERR_CAPACITY, "the radius brings " + std::to_string(pairs) + " block pairs within reach, max_block_pairs is " +
                                               std::to_string(max_block_pairs) + "; nothing was written");
    if (!d_counts) HIP_TRY(c, t.alloc(&d_counts, sizeof(unsigned int) * n));
    launch_neighbour_counts(c->stream, n, c->planes, c->orig, c->bounds, (const unsigned char*)d_source, r2, cap, d_counts);
    launch_neighbour_apply(c->stream, n, d_counts, count_min, count_max, op, (unsigned char*)d_selection, d_count);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (count_out) *count_out = count;
    return SPLAT_OK;
}

// The pick reads the scene as the selections do, on the whole target.  What it allocates goes with the call: one buffer that
// holds the pixels, a counter and a front key per pixel, and a list of max_hits entries per pixel.
int splat_pick_device(splat_ctx* c, const splat_pick_query* q, const splat_camera* cam, uint32_t n_pixels, const int32_t* pixels_xy,
                      const void* d_mask, void* d_results, void* d_layers, void* producer_stream) {
    // (the arguments are judged before the context is looked at, as the PLY entry points do it)
    if (const char* why = pick_refusal(q, cam, n_pixels, pixels_xy, d_results, d_layers)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (n_pixels == 0) return SPLAT_OK;
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to pick from");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    SelectView v = select_view(c, cam);
    v.W = (int)cam->w; v.H = (int)cam->h;
    int4 bound = make_int4(v.W, v.H, -1, -1);                   // x0 y0 x1 y1 of all the queries
    for (uint32_t p = 0; p < n_pixels; ++p) {
        bound.x = std::min(bound.x, pixels_xy[2 * p]); bound.z = std::max(bound.z, pixels_xy[2 * p]);
        bound.y = std::min(bound.y, pixels_xy[2 * p + 1]); bound.w = std::max(bound.w, pixels_xy[2 * p + 1]);
    }
    // one temporary: per pixel a front key and a list of max_hits keys (8 bytes each), then the pixels themselves (8), then a
    // counter and the list's alphas (4 each); the front keys and the counters are zeroed
    const size_t np_ = n_pixels, mh = q->max_hits;
    const size_t keys_bytes = 8u * np_ * (1u + mh), words_bytes = 4u * np_ * (1u + mh);
    Temps t(c);
    unsigned char* d_tmp = nullptr;
    static_assert(sizeof(int2) == 8, "the pixels keep the 8-byte alignment of what lies before them");
    HIP_TRY(c, t.alloc(&d_tmp, keys_bytes + sizeof(int2) * np_ + words_bytes));
    PickTemps pt{};
    pt.fronts = (unsigned long long*)d_tmp;
    pt.list_key = pt.fronts + np_;
    int2* const d_pixels = (int2*)(d_tmp + keys_bytes);
    pt.counts = (unsigned int*)(d_tmp + keys_bytes + sizeof(int2) * np_);
    pt.list_alpha = (float*)(pt.counts + np_);
    HIP_TRY(c, hipMemcpyAsync(d_pixels, pixels_xy, sizeof(int2) * np_, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(pt.fronts, 0, 8u * np_, c->stream));
    HIP_TRY(c, hipMemsetAsync(pt.counts, 0, 4u * np_, c->stream));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_pick(c->stream, c->n, c->planes, c->orig, (const unsigned char*)d_mask, v, *q, n_pixels, d_pixels, bound, pt, d_results, d_layers);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

// The visibility query reads the scene's values, but through a view's tile lists: the scheduler bins the view outside any frame
// (bin_view_for_query: slot 0's records and tile tables, key buffers of the call's own, freed here) and the kernel walks them.
int splat_visibility_device(splat_ctx* c, const splat_visibility_query* q, const splat_camera* cam, const void* d_pixel_mask,
                            const void* d_mask, void* d_pixels, void* d_max_weight, void* d_weight_sum, void* producer_stream) {
    // (the arguments are judged before the context is looked at, as the pick does it)
    if (const char* why = visibility_refusal(q, cam, d_pixels, d_max_weight, d_weight_sum)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to look at");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const uint64_t n = c->n;
    const int W = (int)cam->w, H = (int)cam->h;
    const int x0 = std::max(q->x0, 0), y0 = std::max(q->y0, 0), x1 = std::min(q->x1, W - 1), y1 = std::min(q->y1, H - 1);
    const bool empty = x0 > x1 || y0 > y1;
    int rc = ctx_quiesce(c);                   // (finish_quiet: behind the frames in flight, whatever the region)
    if (rc != SPLAT_OK) return rc;
    ViewLists v{};
    if (!empty) {
        rc = bin_view_for_query(c, cam, &v);
        if (rc != SPLAT_OK) return rc;
    }
    Temps t(c);
    t.adopt(v.keys); t.adopt(v.keys2);
    HIP_TRY(c, follow_producer(c, producer_stream));
    if (q->op == SPLAT_VIS_SET) {
        if (d_pixels) HIP_TRY(c, hipMemsetAsync(d_pixels, 0, sizeof(unsigned int) * n, c->stream));
        if (d_max_weight) HIP_TRY(c, hipMemsetAsync(d_max_weight, 0, sizeof(float) * n, c->stream));
        if (d_weight_sum) HIP_TRY(c, hipMemsetAsync(d_weight_sum, 0, sizeof(unsigned long long) * n, c->stream));
    }
    if (!empty && v.n_pairs != 0) {
        VisibilityArgs a{};
        a.s = c->stream; a.W = W; a.tiles_x = v.fc.tiles_x; a.y_up = v.fc.y_up; a.sample_half = v.fc.sample_half;
        a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1; a.weight_min = q->weight_min;
        a.offsets = v.offsets; a.lens = v.lens; a.keys = v.keys; a.recs = v.recs; a.rect = v.rect; a.orig = c->orig;
        a.mask = (const unsigned char*)d_mask; a.pixel_mask = (const unsigned char*)d_pixel_mask;
        a.pixels = (unsigned int*)d_pixels; a.max_weight = (float*)d_max_weight; a.weight_sum = (unsigned long long*)d_weight_sum;
        launch_visibility(a);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

// Counts into a selection: launch_neighbour_apply behind an entry point of its own.  No scene is read.
int splat_select_counts_device(splat_ctx* c, uint64_t n, const void* d_counts, uint32_t count_min, uint32_t count_max, uint32_t op,
                               void* d_selection, uint64_t* count_out, void* producer_stream) {
    if (const char* why = select_counts_refusal(n, d_counts, count_min, count_max, op, d_selection)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (count_out) *count_out = 0;
    if (n == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    Temps t(c);
    unsigned int* d_count = nullptr;
    unsigned int count = 0;
    HIP_TRY(c, t.alloc(&d_count, sizeof(unsigned int)));
    HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(unsigned int), c->stream));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_neighbour_apply(c->stream, n, (const unsigned int*)d_counts, count_min, count_max, op, (unsigned char*)d_selection, d_count);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (count_out) *count_out = count;
    return SPLAT_OK;
}

// Gaussians taken out of the scene by a selection.  The mask is counted as a READ of the scene -- a call that finds nothing
// to remove has been one -- and only then does the call become an edit that changes n: the new scene arrays are made and
// filled while the old scene is whole, the old one and the frame slots' per-Gaussian buffers go after the compaction has
// completed, and from there on a failure leaves no scene, as in an upload.  The order is the old one's without the slots
// that went: nothing is sorted.
int splat_remove_gaussians_device(splat_ctx* c, uint64_t n, const void* d_selection, uint32_t mode, void* d_index_map_out,
                                  uint64_t* n_out, void* producer_stream) {
    // (the arguments are judged before the context is looked at, as the selections do it)
    if (const char* why = remove_refusal(n, d_selection, mode, d_index_map_out, n_out)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to remove from");
    if (n != c->n) return fail(c, SPLAT_ERR_INVALID, "n is not the resident scene's");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    const unsigned char* mask = (const unsigned char*)d_selection;
    unsigned int* d_map = (unsigned int*)d_index_map_out;
    uint64_t n2 = 0;
    SceneGuard guard{c, true, false};          // armed once the old scene has gone
    {
        Temps t(c);
        unsigned int *d_counts = nullptr, *d_blocks = nullptr;
        unsigned int total = 0;
        const uint64_t g = selection_groups(mask, n);
        HIP_TRY(c, t.alloc(&d_counts, sizeof(unsigned int) * (g + 1)));
        HIP_TRY(c, follow_producer(c, producer_stream));
        launch_selection_indices(c->stream, n, mask, nullptr, 0, d_counts);      // (no room for indices: the counts and their scan)
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&total, d_counts + g, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        n2 = mode == SPLAT_REMOVE_UNSELECTED ? (uint64_t)total : n - total;
        if (n2 != n) {
            rc = end_frames_for_edit(c);
            if (rc != SPLAT_OK) return rc;
        }
        if (n2 == n || n2 == 0) {              // nothing to compact: the map alone, the identity or REMOVED_INDEX throughout
            if (d_map) {
                launch_index_map(c->stream, n, mask, d_counts, mode, d_map);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipStreamSynchronize(c->stream));
            }
            if (n2 == 0) free_scene(c);
            *n_out = n2;
            return SPLAT_OK;
        }
        float4* planes2 = nullptr; unsigned int* orig2 = nullptr; BlockBounds* bounds2 = nullptr;
        HIP_TRY(c, t.alloc(&planes2, sizeof(float4) * SCENE_PLANES * n2));
        HIP_TRY(c, t.alloc(&orig2, sizeof(unsigned int) * n2));
        HIP_TRY(c, t.alloc(&bounds2, sizeof(BlockBounds) * ((n2 + 255) / 256)));
        HIP_TRY(c, t.alloc(&d_blocks, sizeof(unsigned int) * ((n + 255) / 256 + 1)));
        if (!d_map) HIP_TRY(c, t.alloc(&d_map, sizeof(unsigned int) * n));
        launch_index_map(c->stream, n, mask, d_counts, mode, d_map);
        launch_compact_scene(c->stream, n, n2, c->planes, c->orig, d_map, d_blocks, planes2, orig2);
        launch_plane_bounds(c->stream, n2, planes2, nullptr, bounds2);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // the old scene goes, with the inverse and the host copy of its order; the new arrays take its place
        free_scene(c);
        guard.armed = true;
        c->planes = t.keep(planes2); c->orig = t.keep(orig2); c->bounds = t.keep(bounds2);
        HIP_TRY(c, alloc_slot_buffers(c, n2));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    scene_installed(c, n2);
    guard.armed = false;
    *n_out = n2;
    return SPLAT_OK;
}

// Gaussians added behind the resident ones: the removal's opposite, and like it an edit that changes n.  The new arrays of
// n + m slots are made and filled while the old scene is whole -- the resident slots copied, the new rows sorted among
// themselves and packed behind them -- and then take its place as a removal's do.  Nothing resident is sorted: the blocks
// wholly below slot n keep their bounds, the others are made again from the new planes.
int splat_append_gaussians_device(splat_ctx* c, uint64_t n, uint64_t m, const void* d_pos4, const void* d_cov3d, const void* d_opacity,
                                  const void* d_sh, uint64_t* n_out, void* producer_stream) {
    // (the arguments are judged before the context is looked at, as the removal does it)
    if (const char* why = append_refusal(n, m, d_pos4, d_cov3d, d_opacity, d_sh, n_out)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to append to (an empty context takes an upload)");
    if (n != c->n) return fail(c, SPLAT_ERR_INVALID, "n is not the resident scene's");
    if (m == 0) { *n_out = n; return SPLAT_OK; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    rc = end_frames_for_edit(c);
    if (rc != SPLAT_OK) return rc;
    const uint64_t n2 = n + m, nb2 = (n2 + 255) / 256, whole = n / 256;      // whole: the blocks that lie below slot n altogether
    const float* pos4 = (const float*)d_pos4;
    SceneGuard guard{c, true, false};          // armed once the old scene has gone
    {
        Temps t(c);
        float4* planes2 = nullptr; unsigned int* orig2 = nullptr; BlockBounds* bounds2 = nullptr;
        uint32_t* d_sort = nullptr; unsigned char *d_small = nullptr, *d_dirty = nullptr;
        HIP_TRY(c, t.alloc(&planes2, sizeof(float4) * SCENE_PLANES * n2));
        HIP_TRY(c, t.alloc(&orig2, sizeof(unsigned int) * n2));
        HIP_TRY(c, t.alloc(&bounds2, sizeof(BlockBounds) * nb2));
        HIP_TRY(c, t.alloc(&d_sort, sizeof(uint32_t) * 4 * m));
        HIP_TRY(c, t.alloc(&d_small, scene_order_small_bytes(m)));
        HIP_TRY(c, t.alloc(&d_dirty, nb2));
        HIP_TRY(c, follow_producer(c, producer_stream));
        launch_scene_order(c->stream, m, pos4, d_sort, d_small, orig2 + n);
        launch_grow_scene(c->stream, n, n2, c->planes, c->orig, planes2, orig2);
        launch_pack_append(c->stream, n, m, pos4, (const float*)d_cov3d, (const float*)d_opacity, (const float*)d_sh, planes2, orig2);
        if (whole) {
            HIP_TRY(c, hipMemcpyAsync(bounds2, c->bounds, sizeof(BlockBounds) * whole, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemsetAsync(d_dirty, 0, whole, c->stream));
        }
        HIP_TRY(c, hipMemsetAsync(d_dirty + whole, 1, nb2 - whole, c->stream));
        launch_plane_bounds(c->stream, n2, planes2, d_dirty, bounds2);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // the old scene goes, with the inverse and the host copy of its order; the new arrays take its place
        free_scene(c);
        guard.armed = true;
        c->planes = t.keep(planes2); c->orig = t.keep(orig2); c->bounds = t.keep(bounds2);
        HIP_TRY(c, alloc_slot_buffers(c, n2));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    scene_installed(c, n2);
    guard.armed = false;
    *n_out = n2;
    return SPLAT_OK;
}

// The resident scene put into the order a fresh upload of its current values would have.  The order is made first, as a
// READ of the scene -- a call that finds every slot where it belongs has been one -- and only then does the call become
// an edit: the planes are gathered into new arrays while the old scene is whole, and those take its place as a removal's do.
int splat_reorder_scene_device(splat_ctx* c, uint64_t* moved_out) {
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to reorder");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    const uint64_t n = c->n;
    unsigned long long moved = 0;
    SceneGuard guard{c, true, false};          // armed once the old scene has gone
    {
        Temps t(c);
        float* d_pos = nullptr; uint32_t* d_sort = nullptr; unsigned char* d_small = nullptr;
        unsigned int* orig2 = nullptr; unsigned long long* d_moved = nullptr;
        HIP_TRY(c, t.alloc(&orig2, sizeof(unsigned int) * n));
        HIP_TRY(c, t.alloc(&d_pos, sizeof(float) * 4 * n));
        HIP_TRY(c, t.alloc(&d_sort, sizeof(uint32_t) * 4 * n));
        HIP_TRY(c, t.alloc(&d_small, scene_order_small_bytes(n)));
        HIP_TRY(c, t.alloc(&d_moved, sizeof(unsigned long long)));
        HIP_TRY(c, hipMemsetAsync(d_moved, 0, sizeof(unsigned long long), c->stream));
        launch_unpack_scene(c->stream, n, SPLAT_FIELD_POS, d_pos, nullptr, nullptr, nullptr, c->orig, c->planes);
        launch_scene_order(c->stream, n, d_pos, d_sort, d_small, orig2);
        launch_order_moved(c->stream, n, c->orig, orig2, d_moved);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&moved, d_moved, sizeof moved, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (moved == 0) {
            if (moved_out) *moved_out = 0;
            return SPLAT_OK;
        }
        rc = end_frames_for_edit(c);
        if (rc != SPLAT_OK) return rc;
        // the sort's arrays have served: they go before the second set of planes is made
        t.release(d_pos);
        t.release(d_sort);
        t.release(d_small);
        float4* planes2 = nullptr; BlockBounds* bounds2 = nullptr;
        HIP_TRY(c, t.alloc(&planes2, sizeof(float4) * SCENE_PLANES * n));
        HIP_TRY(c, t.alloc(&bounds2, sizeof(BlockBounds) * ((n + 255) / 256)));
        HIP_TRY(c, ensure_inverse(c));
        launch_permute_scene(c->stream, n, c->planes, c->inv, orig2, planes2);
        launch_plane_bounds(c->stream, n, planes2, nullptr, bounds2);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        free_scene(c);
        guard.armed = true;
        c->planes = t.keep(planes2); c->orig = t.keep(orig2); c->bounds = t.keep(bounds2);
        HIP_TRY(c, alloc_slot_buffers(c, n));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    scene_installed(c, n);
    guard.armed = false;
    if (moved_out) *moved_out = moved;
    return SPLAT_OK;
}

int splat_decode_ply_device(splat_ctx* c, const splat_ply_layout* lay, const void* d_rows, void* d_pos4, void* d_scales3,
                            void* d_opacity, void* d_rot4, void* d_sh, void* producer_stream) {
    // (the arguments are judged before the context is looked at, and before any HIP call: without a context the reason is
    // what splat_last_error(NULL) reports)
    const char* why = nullptr;
    if (!ply_layout_ok(lay, &why)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (lay->n == 0) return SPLAT_OK;
    if (!d_rows || !d_pos4 || !d_scales3 || !d_opacity || !d_rot4 || !d_sh) return fail(c, SPLAT_ERR_INVALID, "NULL pointer");
    if (((uintptr_t)d_pos4 & 15u) || (((uintptr_t)d_scales3 | (uintptr_t)d_opacity | (uintptr_t)d_rot4 | (uintptr_t)d_sh) & 3u))
        return fail(c, SPLAT_ERR_INVALID, "output buffer misaligned (pos4: 16 bytes, the others: 4)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, ply_decode_now(c, *lay, d_rows, (float*)d_pos4, (float*)d_scales3, (float*)d_opacity, (float*)d_rot4, (float*)d_sh, producer_stream));
    return SPLAT_OK;
}

int splat_upload_ply_device(splat_ctx* c, const splat_ply_layout* lay, const void* d_rows, int32_t compute_cov3d, void* producer_stream) {
    const char* why = nullptr;
    if (!ply_layout_ok(lay, &why)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (lay->n == 0) return splat_upload_scene_device(c, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!d_rows) return fail(c, SPLAT_ERR_INVALID, "NULL pointer");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const uint64_t n = lay->n;
    // The old scene stays resident under the decode, as it always has (the peak: old scene + the six buffers below), so its
    // frames have not ended yet: a failure in here takes it away as an empty upload would.
    SceneGuard guard{c, false};
    Temps t(c);
    float *d_pos = nullptr, *d_sc = nullptr, *d_op = nullptr, *d_rot = nullptr, *d_sh = nullptr, *d_cov = nullptr;
    HIP_TRY(c, t.alloc(&d_pos, sizeof(float) * 4 * n));
    HIP_TRY(c, t.alloc(&d_sc, sizeof(float) * 3 * n));
    HIP_TRY(c, t.alloc(&d_op, sizeof(float) * n));
    HIP_TRY(c, t.alloc(&d_rot, sizeof(float) * 4 * n));
    HIP_TRY(c, t.alloc(&d_sh, sizeof(float) * 48 * n));
    HIP_TRY(c, t.alloc(&d_cov, sizeof(float) * 9 * n));
    // cov3d first, on the same stream: K0 behind the decode (GaussianList::from_vec), or zeros (Gaussian::new)
    HIP_TRY(c, ply_decode_now(c, *lay, d_rows, d_pos, d_sc, d_op, d_rot, d_sh, producer_stream));
    if (compute_cov3d) {
        launch_cov3d(c->stream, n, d_sc, d_rot, d_cov);
        HIP_TRY(c, hipGetLastError());
    } else {
        HIP_TRY(c, hipMemsetAsync(d_cov, 0, sizeof(float) * 9 * n, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // scales and rotations have served: they go before the upload makes the scene's buffers; the other four it reads
    t.release(d_sc);
    t.release(d_rot);
    guard.armed = false;           // (the upload has a guard of its own)
    return splat_upload_scene_device(c, n, d_pos, d_cov, d_op, d_sh, nullptr);
}

// The inverses of splat_decode_ply_device: the resident scene as PLY vertex rows in the caller's device buffer.  They READ
// the scene as splat_read_*_device do -- behind the frames in flight, nothing of a frame's state touched -- and find a row's
// slot the same way (ensure_inverse).  The arguments are judged before the context is looked at.
int splat_encode_ply_scene_device(splat_ctx* c, const splat_ply_layout* lay, void* d_rows_out) {
    if (const char* why = ply_encode_refusal(lay, d_rows_out)) return fail(c, SPLAT_ERR_INVALID, why);
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (lay->n != c->n) return fail(c, SPLAT_ERR_INVALID, "layout->n is not the resident scene's");
    if (c->n == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    HIP_TRY(c, ensure_inverse(c));
    launch_ply_encode(c->stream, c->n, c->n, nullptr, *lay, c->inv, c->planes, d_rows_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

int splat_encode_ply_gaussians_device(splat_ctx* c, uint64_t k, const void* d_index, const splat_ply_layout* lay, void* d_rows_out,
                                      void* producer_stream) {
    if (const char* why = ply_encode_refusal(lay, d_rows_out)) return fail(c, SPLAT_ERR_INVALID, why);
    if (lay->n != k) return fail(c, SPLAT_ERR_INVALID, "layout->n is not k");
    if (k && !d_index) return fail(c, SPLAT_ERR_INVALID, "NULL d_index");
    if (!c) return fail(c, SPLAT_ERR_INVALID, "NULL context");
    if (k == 0) return SPLAT_OK;
    if (c->n == 0) return fail(c, SPLAT_ERR_NO_SCENE, "no resident scene to encode");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = ctx_quiesce(c);
    if (rc != SPLAT_OK) return rc;
    const unsigned int* index = (const unsigned int*)d_index;
    HIP_TRY(c, ensure_inverse(c));
    HIP_TRY(c, follow_producer(c, producer_stream));
    unsigned int bad = 0;
    HIP_TRY(c, count_bad_indices(c, k, index, &bad));
    if (bad) return fail(c, SPLAT_ERR_INVALID, "d_index: an index is not below n; nothing was written");
    launch_ply_encode(c->stream, c->n, k, index, *lay, c->inv, c->planes, d_rows_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

// (debug, not part of the ABI)  Device time of the decode, the sequential sum and the subtraction inside the most recent
// splat_decode_ply_device / splat_upload_ply_device, in milliseconds.
int splat_debug_ply_ms(splat_ctx* c, double ms[3]) {
    if (!c || !ms) return SPLAT_ERR_INVALID;
    for (int k = 0; k < 3; ++k) ms[k] = c->ply_ms[k];
    return SPLAT_OK;
}

int splat_get_scene_layout(splat_ctx* c, uint32_t* orig_out, uint64_t n, float* bounds_out, uint64_t n_blocks) {
    if (!c) return SPLAT_ERR_INVALID;
    if (n != c->n || n_blocks != (c->n + 255) / 256) return fail(c, SPLAT_ERR_INVALID, "scene layout size mismatch");
    if (n == 0) return SPLAT_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    static_assert(sizeof(BlockBounds) == 8 * sizeof(float), "bounds_out is 8 floats per block");
    if (orig_out) HIP_TRY(c, hipMemcpy(orig_out, c->orig, sizeof(unsigned int) * n, hipMemcpyDeviceToHost));
    if (bounds_out) HIP_TRY(c, hipMemcpy(bounds_out, c->bounds, sizeof(BlockBounds) * n_blocks, hipMemcpyDeviceToHost));
    return SPLAT_OK;
}

int splat_compute_cov3d(splat_ctx* c, uint64_t n, const float* scales3, const float* rot4, float* cov3d_out) {
    if (!c) return SPLAT_ERR_INVALID;
    if (n == 0) return SPLAT_OK;
    if (!scales3 || !rot4 || !cov3d_out) return fail(c, SPLAT_ERR_INVALID, "NULL pointer");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    Temps t(c);
    float *d_s = nullptr, *d_r = nullptr, *d_o = nullptr;
    HIP_TRY(c, t.alloc(&d_s, sizeof(float) * 3 * n));
    HIP_TRY(c, t.alloc(&d_r, sizeof(float) * 4 * n));
    HIP_TRY(c, t.alloc(&d_o, sizeof(float) * 9 * n));
    HIP_TRY(c, hipMemcpyAsync(d_s, scales3, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_r, rot4, sizeof(float) * 4 * n, hipMemcpyHostToDevice, c->stream));
    launch_cov3d(c->stream, n, d_s, d_r, d_o);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cov3d_out, d_o, sizeof(float) * 9 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

int splat_compute_cov3d_device(splat_ctx* c, uint64_t n, const void* d_scales3, const void* d_rot4, void* d_cov3d_out,
                               void* producer_stream) {
    if (!c) return SPLAT_ERR_INVALID;
    if (n == 0) return SPLAT_OK;
    if (!d_scales3 || !d_rot4 || !d_cov3d_out) return fail(c, SPLAT_ERR_INVALID, "NULL pointer");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, follow_producer(c, producer_stream));
    launch_cov3d(c->stream, n, (const float*)d_scales3, (const float*)d_rot4, (float*)d_cov3d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

}  // extern "C"
