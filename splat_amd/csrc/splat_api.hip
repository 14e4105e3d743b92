// splat_api.hip -- C ABI (include/splat_hip.h) over the gfx950 kernels.  Host side only:
// buffer ownership, per-frame constants, launch sequence, HIP-event timing, error reporting.
// The entry points that put values into the resident scene (uploads, PLY, edits, K0) are splat_scene.hip's; the context both
// files share is splat_context.h.
//
// Frames overlap on the device (SPLAT_PIPELINE): per-frame buffers live in SLOTS used in rotation; preprocess +
// scan + sort of later frames run on internal high-priority streams into the next slots while frame N composites
// on the caller's stream (fork/join = two events per frame; nothing is skipped or reused between frames).
//   1  one stream, no overlap
//   2  the chain (K1, scan, sort) of frame N+1 on the bin stream under the compositor of frame N
//   3  the sort on a stream of its own (it starves beside the other two: no gain)
//   4, 5  three / four slots on the two streams of mode 2 (+0..2 %)
//   6  (default) four slots, the chains of consecutive frames on alternating streams: with one chain at a time the
//      frame time is the chain's length under contention; with two the compositor is the bound (C3 +4 %, C1 +10 %)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "splat_context.h"

using namespace splat;

static thread_local std::string g_create_error;
static std::mutex g_ledger_mu;
static std::unordered_map<void*, std::pair<splat_ctx*, size_t>> g_ledger;      // device allocation -> (context, bytes)

namespace splat {
CommState** ctx_comm_slot(splat_ctx* c) { return &c->comm; }
hipStream_t ctx_stream(splat_ctx* c) { return c->stream; }
// the stream the most recent frame's compositor was enqueued on: work that must follow THAT frame (the gather of its rows,
// the copy of its pixels) goes there -- and the next frame to the same image follows it on the same lane
hipStream_t frame_stream(splat_ctx* c) { return (c->last_lane && c->comp2) ? c->comp2 : c->stream; }
// Work enqueued BEHIND the most recent frame on its lane that later frames / copies must also follow (the gather of its
// rows): the frame's ring event -- the one every cross-lane hazard wait, join_lanes, the slot-reuse wait and the image
// table use -- is recorded again behind it, so "the frame has ended" includes that work from now on.
int frame_tail(splat_ctx* c) {
    if (c->last_ring < 0 || !c->ring[c->last_ring].used) return SPLAT_OK;
    hipError_t e = hipEventRecord(c->ring[c->last_ring].e[7], frame_stream(c));
    if (e != hipSuccess) { c->err = std::string("hipEventRecord(frame tail): ") + hipGetErrorString(e); return SPLAT_ERR_HIP; }
    return SPLAT_OK;
}
int ctx_device(const splat_ctx* c) { return c->cfg.device; }
int ctx_fail(splat_ctx* c, int code, const char* msg) { if (c) c->err = msg; return code; }

// (splat_context.h: both host files report and account through these)
int fail(splat_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}
void ledger_add(splat_ctx* c, void* p, size_t bytes) {
    std::lock_guard<std::mutex> g(g_ledger_mu);
    g_ledger[p] = {c, bytes};
    c->dev_bytes += bytes;
    c->dev_bytes_peak = std::max(c->dev_bytes_peak, c->dev_bytes);
}
void ledger_del(void* p) {
    std::lock_guard<std::mutex> g(g_ledger_mu);
    auto it = g_ledger.find(p);
    if (it == g_ledger.end()) return;
    it->second.first->dev_bytes -= it->second.second;
    g_ledger.erase(it);
}
}  // namespace splat

namespace {

const float* ev_times(const EvSet& s, float t[N_TIMES]) {
    static const int pairs[N_TIMES][2] = {{0, 1}, {1, 2}, {8, 3}, {3, 4}, {5, 6}, {6, 7}};
    for (int k = 0; k < N_TIMES; ++k) {
        t[k] = 0.f;
        if (s.retained && k < 4) continue;      // (events 0-4 and 8 of this ring entry are an older frame's: a retained frame bins and orders nothing)
        (void)hipEventElapsedTime(&t[k], s.e[pairs[k][0]], s.e[pairs[k][1]]);
    }
    return t;
}

void harvest(splat_ctx* c, int r) {
    EvSet& s = c->ring[r];
    if (!s.used) return;
    (void)hipEventSynchronize(s.e[7]);
    if (s.timed) {
        float t[N_TIMES];
        ev_times(s, t);
        for (int k = 0; k < N_TIMES; ++k) c->acc_ms[k] += t[k];
        c->acc_frames++;
    }
    const FrameStatus& st = c->h_status[r];
    if (st.overflow) c->frames_dropped++;
    if (st.overflow == 1) c->overflow_want = std::max<uint64_t>(c->overflow_want, st.n_pairs);
    if (st.overflow == 2) c->bucket_overflow = true;           // a tile's list outgrew its region: the layouts are stale
    if (st.overflow == 2 || st.redone == 1u) c->pol.redo_armed = SPLAT_POLICY_REDO_RUN;  // ... or did and was binned again on the device: keep the redo launches on
    if (st.layout_total > c->cap) c->layout_want = std::max<uint64_t>(c->layout_want, st.layout_total);   // the regions were cut off
    if (st.overflow == 3) c->sort_grid_miss = true;
    if (st.overflow == 4) c->keys2_want = std::max<uint64_t>(c->keys2_want, st.n_long_keys);
    if (st.overflow == 0 || st.overflow == 3) { c->sort_hint = true; c->hint_ge8192 = st.n_ge8192; c->hint_ge2048 = st.n_ge2048; c->hint_ge16384 = st.n_ge16384; }
    if (st.overflow == 0) { c->hint_pairs = st.n_pairs; c->hint_maxlen = st.max_tile_len; c->hint_large = st.n_large; c->hint_window = st.n_window; }
    s.used = false;
}

// Page-locked host ranges this library made (splat_host_alloc / splat_host_register): start -> bytes.  The zero-copy frame
// stores W*H*4 bytes through the device mapping of `argb_out`; the mapping must cover all of them (a caller that
// registered a slab's worth of a larger image got a GPU page fault instead of the copy path).  A range the table does not
// know (locked by the caller's own hipHostMalloc / hipHostRegister, a framework's pinned tensor) is asked of the runtime.
static std::mutex g_host_mu;
static std::unordered_map<const char*, size_t> g_host_ranges;
static void host_range_add(const void* p, size_t bytes) { std::lock_guard<std::mutex> g(g_host_mu); g_host_ranges[(const char*)p] = bytes; }
static void host_range_del(const void* p) { std::lock_guard<std::mutex> g(g_host_mu); g_host_ranges.erase((const char*)p); }
static bool host_range_is_locked(const void* host, void* dev, size_t bytes) {
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        const char* lo = (const char*)host;
        for (const auto& r : g_host_ranges)
            if (r.first <= lo && lo < r.first + r.second) return lo + bytes <= r.first + r.second;      // (ours: the table decides)
    }
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dev) == hipSuccess && base != nullptr &&
        (const char*)dev >= (const char*)base && (const char*)dev + bytes <= (const char*)base + size)
        return true;
    (void)hipGetLastError();
    return false;
}

// Device -> host copy of image rows behind a frame.  A destination of which only a PART is page-locked (ADVICE r5's case: the
// caller registered a slab's worth of a larger image) is refused whole by hipMemcpyAsync (invalid argument): it is copied in
// pieces cut at the borders of the locked ranges this library knows, and a piece the runtime still refuses goes through a
// page-locked staging buffer.  The usual destination -- wholly locked or wholly pageable -- is one call as before.
static hipError_t copy_to_host_image(uint32_t* dst, const uint32_t* src, size_t bytes, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
    if (e != hipErrorInvalidValue) return e;
    (void)hipGetLastError();
    std::vector<size_t> cuts{0, bytes};
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        const char* lo = (const char*)dst;
        for (const auto& r : g_host_ranges)
            for (const char* edge : {r.first, r.first + r.second})
                if (edge > lo && edge < lo + bytes) cuts.push_back((size_t)(edge - lo));
    }
    std::sort(cuts.begin(), cuts.end());
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const size_t off = cuts[k], len = cuts[k + 1] - cuts[k];
        if (!len) continue;
        e = hipMemcpyAsync((char*)dst + off, (const char*)src + off, len, hipMemcpyDeviceToHost, stream);
        if (e == hipErrorInvalidValue) {
            (void)hipGetLastError();
            void* stage = nullptr;
            if ((e = hipHostMalloc(&stage, len)) != hipSuccess) return e;
            e = hipMemcpyAsync(stage, (const char*)src + off, len, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e == hipSuccess) std::memcpy((char*)dst + off, stage, len);
            (void)hipHostFree(stage);
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The frame policy's memory speaks of lists that no longer exist (another scene, target, slab, key-buffer layout) or of
// thresholds that changed (an option): forget it.  Statuses of frames still in the ring stay where they are; ring_kind = 0
// makes the policy ignore them ('binned twice' words of an earlier scene could arm 64 count-first frames on the next).
// RETAINED LISTS (include/splat_retain.h): whatever changes what K1, the scan or the ordering of a frame would read or
// produce ends the retained set -- the next frame's decision sees another epoch.
void bump_epoch(splat_ctx* c) { ++c->bin_epoch; }

void reset_policy(splat_ctx* c) {
    bump_epoch(c);
    c->pol.still_frames = 0; c->pol.last_cam_hash = 0;
    c->pol.count_first_left = 0; c->pol.redo_armed = 0;
    std::memset(c->pol.ring_kind, 0, sizeof c->pol.ring_kind);
}

int sync_all(splat_ctx* c) {
    if (c->bin_stream) HIP_TRY(c, hipStreamSynchronize(c->bin_stream));
    if (c->sort_stream) HIP_TRY(c, hipStreamSynchronize(c->sort_stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));      // (lane 1 is this stream too)
    return SPLAT_OK;
}

// the stream (and events) of splat_render_stream's device -> host copies
hipError_t ensure_copy_stream(splat_ctx* c) {
    if (c->copy_stream) return hipSuccess;
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (int k = 0; k < splat_ctx::S_IMGS && e == hipSuccess; ++k) {
        if (!c->s_rendered[k]) e = hipEventCreateWithFlags(&c->s_rendered[k], hipEventDisableTiming);
        if (e == hipSuccess && !c->s_copied[k]) e = hipEventCreateWithFlags(&c->s_copied[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) { if (st) (void)hipStreamDestroy(st); return e; }      // (events made so far are reused by the next attempt, destroyed with the context)
    c->copy_stream = st;
    return hipSuccess;
}

// The copy entry points run on the context's stream: they follow what the second lane still holds as well.
hipError_t join_lanes(splat_ctx* c) {
    if (!c->comp2 || c->lane[1].seq == 0 || c->lane[1].ring < 0) return hipSuccess;
    return hipStreamWaitEvent(c->stream, c->ring[c->lane[1].ring].e[7], 0);
}

// the second compositor lane exists from the first time something may use it
int ensure_lane(splat_ctx* c) {
    if (c->comp2 || c->pipeline == 0) return SPLAT_OK;        // (one stream for everything: no lanes)
    // Lane 1 IS the copy stream of splat_render_stream.  HIP multiplexes its streams onto four hardware queues, and the
    // context already has four (the caller's, two binning chains, the copy stream): a fifth shares a queue with a busy
    // one -- measured both ways round, whichever of the two was created later lost a third of its rate (streamed C3
    // 2570 -> 1840 frames/s, or the swap chain on C2 8100 -> 6060).  The two are never busy together: streamed frames
    // stay on lane 0 (render_device_impl), so the copy stream carries either copies or lane-1 compositors.
    HIP_TRY(c, ensure_copy_stream(c));
    c->comp2 = c->copy_stream;
    return SPLAT_OK;
}

// the context's scene and hint table as the launches' argument blocks name them (a table about to be made: its stride given)
SceneArgs scene_of(const splat_ctx* c) { return {c->n, c->planes, c->orig, c->bounds}; }
HintTable hint_table(const splat_ctx* c, size_t stride) { return {c->need_hint, stride}; }
HintTable hint_table(const splat_ctx* c) { return hint_table(c, c->m_alloc); }

int ensure_bins(splat_ctx* c, unsigned int m) {
    if (m + 1 <= c->m_alloc) return SPLAT_OK;
    int rc = sync_all(c);
    if (rc != SPLAT_OK) return rc;
    c->m_alloc = 0;
    bump_epoch(c);                         // (the slots' tile tables are made again)
    c->sort_hint = false;                  // another target geometry: the list-length profile is unknown again
    dfree(c->zero_layout);
    HIP_TRY(c, dmalloc(c, &c->zero_layout, sizeof(unsigned int) * (size_t)(m + 1)));
    HIP_TRY(c, fill_now(c->zero_layout, 0, sizeof(unsigned int) * (size_t)(m + 1)));
    dfree(c->need_hint);
    dfree(c->stage_nv); dfree(c->stage_mask);      // (made again, for the new tile count, by the next writer: composite_frame)
    HIP_TRY(c, dmalloc(c, &c->need_hint, hint_table(c, (size_t)(m + 1)).bytes()));
    HIP_TRY(c, fill_now(c->need_hint, 0, hint_table(c, (size_t)(m + 1)).bytes()));
    for (Slot& s : c->slots) {
        dfree(s.counts); dfree(s.offsets); dfree(s.cursor); dfree(s.order); dfree(s.lens); dfree(s.counts_b); dfree(s.lay_a); dfree(s.lay_b);
        dfree(s.near_m); dfree(s.redo_layout); dfree(s.redo_cursors); dfree(s.off2);
        s.layout_valid = false; s.flip = 0;
        HIP_TRY(c, dmalloc(c, &s.off2, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.near_m, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.redo_layout, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.redo_cursors, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.counts_b, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.lay_a, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.lay_b, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.lens, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.counts, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.offsets, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.cursor, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, dmalloc(c, &s.order, sizeof(unsigned int) * (size_t)(m + 1)));
        HIP_TRY(c, fill_now(s.counts, 0, sizeof(unsigned int) * (size_t)(m + 1)));
    }
    c->m_alloc = m + 1;
    return SPLAT_OK;
}

int slots_in_use(const splat_ctx* c);

// depth / pixel rectangle / visible list per Gaussian and frame slot (16 bytes x N x slots): what the COUNTING flavour of K1
// hands to K2 -- two-pass binning, splat_tile_row_loads, splat_get_records.  A one-pass frame keeps all three in registers,
// so they exist from the first call that needs them (the slots the caller names), not from the upload.
int ensure_two_pass_buffers(splat_ctx* c, Slot& s) {
    if (s.depth || c->n == 0) return SPLAT_OK;
    hipError_t e = dmalloc(c, &s.depth, sizeof(float) * c->n);
    if (e == hipSuccess) e = dmalloc(c, &s.rect, sizeof(ushort4) * c->n);
    if (e == hipSuccess) e = dmalloc(c, &s.vislist, sizeof(unsigned int) * c->n);
    if (e != hipSuccess) { dfree(s.depth); dfree(s.rect); dfree(s.vislist); return fail(c, SPLAT_ERR_HIP, std::string("hipMalloc(two-pass buffers): ") + hipGetErrorString(e)); }
    return SPLAT_OK;
}

// keys of at least `want` entries, and a second key buffer of at least `want2`, in every slot that frames rotate through
// (a buffer that is large enough is kept)
int ensure_keys(splat_ctx* c, uint64_t want, uint64_t want2) {
    if (want <= c->cap && want2 <= c->cap2) return SPLAT_OK;
    if (want >= 0xFFFFFFF0ull || want2 >= 0xFFFFFFF0ull) return fail(c, SPLAT_ERR_CAPACITY, "pair count exceeds 2^32");
    int rc = sync_all(c);
    if (rc != SPLAT_OK) return rc;
    want = std::max(want, c->cap); want2 = std::max(want2, c->cap2);
    bump_epoch(c);                         // (the slots' key buffers are made again)
    const bool grow1 = want > c->cap, grow2 = want2 > c->cap2;
    // The last frame's lists stay readable (splat_get_tile_lists): a frame whose regions asked for more than the buffer holds
    // was squeezed into it and is complete, and the growth it asked for comes behind it (finish_frame) -- its slot's keys are
    // carried into the new buffer.
    const uint64_t old_cap = c->cap;
    unsigned long long* kept = nullptr;
    if (grow1 && c->last_slot >= 0 && old_cap) std::swap(kept, c->slots[c->last_slot].keys);
    if (grow1) { c->cap = 0; for (Slot& s : c->slots) dfree(s.keys); }
    if (grow2) { c->cap2 = 0; for (Slot& s : c->slots) dfree(s.keys2); }
    for (int k = 0; k < slots_in_use(c); ++k) {
        Slot& s = c->slots[k];
        hipError_t e = hipSuccess;
        if (grow1) e = dmalloc(c, &s.keys, sizeof(unsigned long long) * want);
        if (e == hipSuccess && kept && k == c->last_slot) {
            e = hipMemcpy(s.keys, kept, sizeof(unsigned long long) * old_cap, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (the context's streams do not wait for the default stream: fill_now)
            dfree(kept);
        }
        if (e == hipSuccess && grow2) e = dmalloc(c, &s.keys2, sizeof(unsigned long long) * want2);
        if (e != hipSuccess) {
            // (all or nothing: a half-made set would leave slots without buffers behind capacities that say otherwise)
            for (Slot& t : c->slots) { dfree(t.keys); dfree(t.keys2); }
            dfree(kept);
            c->cap = 0; c->cap2 = 0;
            return fail(c, SPLAT_ERR_CAPACITY, std::string("cannot allocate pair buffer: ") + hipGetErrorString(e));
        }
    }
    dfree(kept);                           // (a last slot beyond the slots in use: nothing to carry)
    c->cap = want; c->cap2 = want2;
    return SPLAT_OK;
}

uint64_t default_pair_capacity(const splat_ctx* c) {
    return c->cfg.pair_capacity ? c->cfg.pair_capacity : std::max<uint64_t>(1ull << 22, 16 * c->n);
}
// One-pass binning: four times that while the key buffers of all frame slots together stay under 8 GiB, twice under 64 GiB (C5 --
// 6 M Gaussians at 4K -- would take 24 GB at 64 N for nothing measurable at rest).
// What the tiles' regions do not ask for is handed out to them as room to grow (build_layout), and that room is what a moving
// camera lives on: with 16 N entries the trained-like surface scene's lists (10-13.5 M pairs, regions asking for 1.5 x + 512 a
// tile) left none.  C3s at 3 / 10 degrees a frame: 1450 / 1340 frames/s with 16 N, 1650 / 1340 with 32 N, 1725 / 1460 with 64 N
// (frames no longer binned twice); 36 uncorrelated synchronous poses 602 -> 811 -> 825 frames/s.  2.3 -> 6.1 GB of device
// memory on C3, 14.8 -> 15.4 GB on C5 (32 N), of 288.
uint64_t region_capacity_for(const splat_ctx* c, uint64_t mult) { return std::max<uint64_t>(1ull << 22, mult * c->n); }
// The second key buffer of a one-pass frame slot: room for the lists of more than 2048 keys (the scan hands it out).  12
// entries per Gaussian hold every frame measured (C3's bench pose asks for 5.3 M of 18 M, the surface scene from inside
// for 15 M); a frame that asks for more is skipped once and the buffer grown (finish_frame).
uint64_t default_keys2_capacity(const splat_ctx* c) {
    if (c->knobs.dbg_keys2_entries) return c->knobs.dbg_keys2_entries;      // (tests force the growth path)
    return std::max<uint64_t>(1ull << 22, 12 * c->n);
}
uint64_t default_region_multiplier(splat_ctx* c) {
    if (c->keys_per_gaussian) return c->keys_per_gaussian;
    if (c->region_mult) return c->region_mult;             // (decided once per scene: the query below is a driver call)
    const uint64_t per_entry = 8ull * (uint64_t)slots_in_use(c);               // a key buffer in every frame slot
    const uint64_t GiB = 1ull << 30;
    // 32 entries per Gaussian (64 for scenes of up to half a million Gaussians, where it is a gigabyte: their frames are
    // short, and a frame binned twice shows), 16 beyond 32 GiB.  What the 64 of round 5 bought a camera in motion -- fewer
    // frames binned twice -- the count-first frames of round 6 give it without the room (profiles/r06_motion_probe.txt),
    // for 1.5 GB less on C3.
    uint64_t mult = 16;
    if (64 * c->n * per_entry <= 1 * GiB) mult = 64;
    else if (32 * c->n * per_entry <= 32 * GiB) mult = 32;
    // ... and never more than a quarter of what the device has free right now: a GPU shared with other contexts (eight slab
    // ranks on one device, a host application's own allocations) takes the smaller buffer at once instead of failing the large one
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b != 0)
        while (mult > 16 && region_capacity_for(c, mult) * per_entry > (uint64_t)free_b / 4u) mult >>= 1;
    else (void)hipGetLastError();
    c->region_mult = mult;
    return mult;
}

// One-pass binning (per-tile regions of the key buffer)?  Not when switched off, when the caller fixed the pair capacity
// (exactly sized lists then), or after the key buffers failed to fit.
bool one_pass_wanted(const splat_ctx* c, unsigned int m) {
    return c->use_buckets && !c->cfg.pair_capacity && m != 0 && !c->bucket_failed;
}
constexpr uint64_t KEY_ENTRIES_MAX = 0xfff00000ull - 65536ull;      // (cursors are 32 bits and run past their regions' ends on a frame that overflows: headroom)

int build_frame_const(splat_ctx* c, const splat_camera* cam, FrameConst* fc, unsigned int* n_tiles) {
    if (!cam) return fail(c, SPLAT_ERR_INVALID, "camera is NULL");
    if (!(cam->w >= 1.0f) || !(cam->h >= 1.0f) || cam->w > 65535.0f || cam->h > 65535.0f ||
        cam->w != std::floor(cam->w) || cam->h != std::floor(cam->h))
        return fail(c, SPLAT_ERR_INVALID, "camera w/h must be integers in [1, 65535]");
    std::memcpy(fc->view, cam->view, sizeof fc->view);
    std::memcpy(fc->proj, cam->proj, sizeof fc->proj);
    fc->w = cam->w; fc->h = cam->h;
    fc->htanx = cam->htanx; fc->htany = cam->htany; fc->focal = cam->focal;
    fc->cam[0] = cam->cam_pos[0]; fc->cam[1] = cam->cam_pos[1]; fc->cam[2] = cam->cam_pos[2];
    fc->lowpass = cam->lowpass; fc->sh_dim = cam->sh_dim;
    fc->y_up = c->cfg.y_up; fc->sample_half = c->cfg.sample_half; fc->zclip = c->cfg.zclip;
    fc->zmin = c->cfg.zmin; fc->zmax = c->cfg.zmax;
    fc->early_eps = c->early_eps; fc->early_min = c->early_min; fc->prio_len = c->prio_len;
    fc->close_width = (c->cfg.mode & SPLAT_MODE_FAST) ? c->fast_width : 0.0f;
    fc->early_scan8 = c->early_scan8;
    fc->bucket_cap = 0;
    fc->corrected = (c->cfg.mode & SPLAT_MODE_CORRECTED_PROJECTION) ? 1 : 0;
    fc->redo_only = 0;
    fc->large_tiles = std::max(0, c->large_tiles);
    fc->start_hints = 0;
    fc->start_light = 0;
    // (a singular cov2d needs lowpass == 0 or a non-PSD cov3d; with lowpass == 0 every Gaussian is
    // looked at so that n_singular stays what the reference would have panicked on)
    fc->cull_blocks = (c->cull_blocks && c->bounds && cam->lowpass > 0.0f) ? 1 : 0;
    fc->W = (int)cam->w; fc->H = (int)cam->h;
    fc->tiles_x = (fc->W + TILE - 1) / TILE;
    int tiles_y = (fc->H + TILE - 1) / TILE;
    int r0 = std::max(0, c->slab0), r1 = (c->slab1 < 0) ? tiles_y : std::min(c->slab1, tiles_y);
    if (r1 < r0) r1 = r0;
    fc->tile_row0 = r0; fc->n_tile_rows = r1 - r0;
    fc->row_px0 = r0 * TILE; fc->row_px1 = std::min(r1 * TILE, fc->H);
    *n_tiles = (unsigned int)(fc->tiles_x * fc->n_tile_rows);
    return SPLAT_OK;
}

// What the stages of enqueue_frame share: filled once, as the frame's ring entry, slot, decisions and streams become known.
struct FrameLaunch {
    int r;                      // the frame's entry of the event / status ring
    EvSet* ev;
    bool timed;
    int si;                     // the frame's slot
    Slot* s;
    FrameStatus* d_st;          // (initialised by this frame's scan)
    splat_policy_decision pd;
    hipStream_t bs, ss, cs;     // binning, ordering, compositor
    TileLists lists;
    KeyBuffers keys;
    int retain;                 // SPLAT_RETAIN_*: an ordinary frame, the writer of a retained set, a frame composited from that set
    hipError_t mark(int k, hipStream_t st) const { return timed ? hipEventRecord(ev->e[k], st) : hipSuccess; }
};

// The frame policy's view of the context: its knobs ...
splat_policy_knobs policy_knobs_of(const splat_ctx* c) {
    splat_policy_knobs pk;
    pk.start_hints = c->start_hints | (c->start_refine ? 0 : SPLAT_POLICY_NO_REFINE); pk.count_first = c->count_first; pk.overflow_redo = c->overflow_redo; pk.early_min = c->early_min;
    pk.early_eps = c->early_eps; pk.near_cap = c->near_cap; pk.fused_sort_max = c->fused_sort_max; pk.sort_in_comp = c->sort_in_comp;
    pk.pair_mode = c->pair_mode; pk.pipeline = c->pipeline; pk.tight_grids = c->tight_grids ? 1 : 0;
    pk.large_list_min = c->large_tiles < 0 ? -1 : c->large_list_min; pk.layout_motion = c->layout_motion;
    return pk;
}
// ... and its input: the camera, the slot's regions, the last harvested frame's list profile, the statuses of the frames in flight
splat_policy_input policy_input_of(const splat_ctx* c, const Slot& s, int ring_entry, bool awaited) {
    splat_policy_input pi;
    std::memset(&pi, 0, sizeof pi);
    std::memcpy(pi.view, c->fc.view, sizeof pi.view); std::memcpy(pi.proj, c->fc.proj, sizeof pi.proj);
    pi.w = c->fc.w; pi.h = c->fc.h; pi.htanx = c->fc.htanx; pi.htany = c->fc.htany; pi.focal = c->fc.focal;
    std::memcpy(pi.cam, c->fc.cam, sizeof pi.cam); pi.lowpass = c->fc.lowpass;
    pi.tile_row0 = c->fc.tile_row0; pi.n_tile_rows = c->fc.n_tile_rows;
    pi.frame_idx = c->frame_idx; pi.ring_entry = ring_entry; pi.one_pass = c->fc.bucket_cap ? 1 : 0;
    pi.layout_valid = s.layout_valid ? 1 : 0; pi.layout_cam = s.layout_cam[s.flip];
    pi.awaited = awaited ? 1 : 0; pi.idle = c->idle ? 1 : 0; pi.has_keys2 = s.keys2 != nullptr ? 1 : 0; pi.n_tiles = c->n_tiles;
    pi.sort_hint = c->sort_hint ? 1 : 0; pi.hint_maxlen = c->hint_maxlen; pi.hint_ge2048 = c->hint_ge2048; pi.hint_ge8192 = c->hint_ge8192;
    pi.hint_ge16384 = c->hint_ge16384; pi.hint_pairs = c->hint_pairs; pi.hint_large = c->hint_large; pi.hint_window = c->hint_window;
    for (int q = 0; q < EV_RING; ++q) {      // (the scans of frames in flight write these words to the host: a peek, no wait)
        const volatile FrameStatus* hs = &c->h_status[q];
        pi.status[q].in_flight = c->ring[q].used ? 1u : 0u; pi.status[q].arrived = hs->arrived;
        pi.status[q].overflow = hs->overflow; pi.status[q].redone = hs->redone;
    }
    return pi;
}

// THE BINNING STAGE, on f.bs: the count-first bootstrap, K1 + the large list, the scan (with the next slot's layout), the overflow redo.
int bin_frame(splat_ctx* c, const FrameLaunch& f) {
    Slot& s = *f.s;
    const splat_policy_decision& pd = f.pd;
    hipStream_t bs = f.bs;
    const unsigned int m = c->n_tiles;
    if (c->pipeline) {
        // order this frame's binning after whatever the caller queued before the call (it may have
        // written the scene-independent inputs we read? no -- but it keeps stream semantics intact
        // for a caller that interleaves uploads), and after the compositor that last used the slot
        if (s.used && s.free_ring >= 0) HIP_TRY(c, hipStreamWaitEvent(bs, c->ring[s.free_ring].e[7], 0));
    }
#if SPLAT_K1X == 30 || SPLAT_K1X == 31
    { int rck = ensure_two_pass_buffers(c, s); if (rck != SPLAT_OK) return rck; }      // (the timeline builds stamp into depth / rect)
#endif
    if (!c->fc.bucket_cap) {                               // two-pass binning: K1 counts visible Gaussians into the status before the scan
        int rc2 = ensure_two_pass_buffers(c, s);
        if (rc2 != SPLAT_OK) return rc2;
        HIP_TRY(c, hipMemsetAsync(f.d_st, 0, sizeof(FrameStatus), bs));
    }
    const uint64_t cam_hash = pd.cam_hash;      // (what places the Gaussians on the target: the camera and the slab)
    BinArgs k1{};
    k1.s = bs; k1.knobs = &c->knobs; k1.scene = scene_of(c); k1.fc = c->fc;
    k1.recs = s.recs; k1.depth = s.depth; k1.rect = s.rect; k1.vislist = s.vislist; k1.keys = s.keys; k1.blockinfo = s.blockinfo; k1.status = f.d_st;
    // (no list: K1's blocks expand their close-ups themselves, and only count the large splats)
    k1.large = {pd.use_large_list ? s.large_list : nullptr, s.large_count, (unsigned int)c->n};
    // One-pass binning: the tiles' regions of the key buffer and their cursors.  Normally the layout_kernel of the frame
    // before this one ON THIS STREAM has left them in the slot's other copy (below); a slot without a layout (first
    // frames, a new scene / target / slab, after a frame outgrew a region) counts its pairs first -- K1 against the
    // empty layout drops every key and counts every pair -- and builds regions that fit exactly this camera.
    k1.bin = {s.counts, nullptr};
    if (c->fc.bucket_cap) {
        // COUNT FIRST (pd.count_first): the frame counts its pairs per tile (K1's count flavour: geometry planes only, no SH, no
        // record, no key -- a third of a K1) and bins into regions that fit exactly ITS camera.
        if (pd.count_first != 0) {
            const int into = s.layout_valid ? s.flip : 1;
            HIP_TRY(c, hipMemsetAsync(s.redo_cursors, 0, sizeof(unsigned int) * ((size_t)m + 1), bs));     // (the redo's buffer: a count-first frame has no redo)
            BinArgs count = k1;
            count.bin = {s.redo_cursors, c->zero_layout}; count.count_only = true;
            launch_preprocess(count); launch_bin_large(count);
            LayoutArgs lay{};
            lay.s = bs; lay.m = m; lay.from = count.bin; lay.next = {into ? s.counts_b : s.counts, into ? s.lay_b : s.lay_a};
            lay.key_entries = c->fc.bucket_cap; lay.spare_max = c->region_spare; lay.large_count = s.large_count;
            launch_layout(lay);
            s.flip = into; s.layout_valid = true;
            s.layout_cam[into] = cam_hash;
        }
        k1.bin = {s.flip ? s.counts_b : s.counts, s.flip ? s.lay_b : s.lay_a};
    }
    HIP_TRY(c, f.mark(0, bs));
    launch_preprocess(k1);
    if (c->fc.bucket_cap) launch_bin_large(k1);     // (the large splats K1 listed, tile by tile)
    HIP_TRY(c, f.mark(1, bs));
    c->grid_big = pd.grid_big; c->grid_mid = pd.grid_mid; c->grid_long = pd.grid_long;      // (what the sort launches cover; the scan validates)
    ScanArgs scan{};
    scan.s = bs; scan.knobs = &c->knobs; scan.m = m; scan.bin = k1.bin; scan.lists = f.lists; scan.keys = f.keys; scan.bucket_cap = c->fc.bucket_cap;
    scan.grids = {c->grid_big, c->grid_mid, c->grid_long}; scan.status = f.d_st; scan.host_status = &c->h_status[f.r];
    scan.spare_max = c->region_spare; scan.large_count = s.large_count;
    // (one-pass binning: a second workgroup of the scan's launch builds the regions of the NEXT frame on this binning
    // stream -- two frames on with two chains in flight -- from this frame's lists, into that slot's idle copy)
    if (c->fc.bucket_cap) {
        const int stride = (c->pipeline >= 6) ? 2 : 1;
        Slot& nx = c->slots[(f.si + stride) % slots_in_use(c)];
        const int into = (&nx == &s) ? (s.flip ^ 1) : (nx.layout_valid ? (nx.flip ^ 1) : 1);
        scan.next.to = {into ? nx.counts_b : nx.counts, into ? nx.lay_b : nx.lay_a};
        nx.flip = into; nx.layout_valid = true;
        nx.layout_cam[into] = cam_hash;
    }
    scan.next.tiles_x = (unsigned int)c->fc.tiles_x; scan.next.motion_radius = (unsigned int)pd.layout_radius;
    launch_scan(scan);
    if (pd.redo != 0) {
        // OVERFLOW REDO.  The regions this frame was binned into were sized for another camera (two frames back on a moving
        // path): if the scan above found a list beyond its region, the frame is binned again right here -- regions that
        // fit exactly this camera (from the counts the first pass left), K1, scan -- into copies of their own; if not
        // (the usual case) every one of these launches reads one word and leaves.  Either way the kernels behind see a
        // complete frame: nothing is skipped, nothing to report, nothing for the caller to render again.
        // (No count pass: K1's reservations keep counting past a region's end -- cursor minus region start IS the tile's exact
        // pair count, overflowed or not (the scan's `raw`) -- and the scan leaves cursors and regions alone: the regions that
        // fit this camera are built straight from them.  One K1 where round 5 ran two.)
        // The first pass's argument blocks, with what differs: the redo's own cursors and regions, the gate, no next layout.
        LayoutArgs lay{};
        lay.s = bs; lay.m = m; lay.from = k1.bin; lay.next = {s.redo_cursors, s.redo_layout};
        lay.key_entries = c->fc.bucket_cap; lay.spare_max = c->region_spare; lay.redo_gate = f.d_st;
        launch_layout(lay);
        k1.fc.redo_only = 1; k1.bin = lay.next;
        launch_preprocess(k1); launch_bin_large(k1);
        scan.bin = k1.bin; scan.next = {}; scan.redo_only = true;
        launch_scan(scan);
    }
    HIP_TRY(c, f.mark(2, bs));
    return SPLAT_OK;
}

// THE ORDERING STAGE, on f.ss behind the binning: the emit of two-pass binning, then the near selection or the sort launches.
int order_frame(splat_ctx* c, const FrameLaunch& f) {
    Slot& s = *f.s;
    const splat_policy_decision& pd = f.pd;
    hipStream_t ss = f.ss;
    const unsigned int m = c->n_tiles;
    if (ss != f.bs) {
        HIP_TRY(c, hipEventRecord(s.ev_binned, f.bs));
        HIP_TRY(c, hipStreamWaitEvent(ss, s.ev_binned, 0));
    }
    HIP_TRY(c, f.mark(8, ss));
    if (!c->fc.bucket_cap) {    // one-pass binning placed the keys in K1
        EmitArgs emit{};
        emit.s = ss; emit.scene = scene_of(c); emit.fc = c->fc; emit.depth = s.depth; emit.rect = s.rect; emit.vislist = s.vislist;
        emit.cursor = s.cursor; emit.keys = s.keys; emit.status = f.d_st;
        launch_emit(emit);
    }
    HIP_TRY(c, f.mark(3, ss));
    if (pd.near_cap) {     // near selection: the nearest keys of the long lists instead of the sort launches
        // Its workgroups: an eighth as many as tiles, each walking the longest-first order with that stride until the lists get
        // short -- a frame in the pipeline has 0.3 ms of slack in front of its compositor, and fewer resident selections leave
        // the previous frame's compositor its LDS (C3 +2 %, C3s +4 %; a sixteenth: C3 +1 %, C3s -1 %; a 64th: -15 %).  A frame
        // the caller waits for gets a workgroup per long list (their number a frame ago, plus an eighth).
        const HintTable hints = hint_table(c);
        SelectArgs sel{};
        sel.s = ss; sel.knobs = &c->knobs; sel.n_tiles = m; sel.lists = f.lists; sel.keys = f.keys; sel.status = f.d_st; sel.orig = c->orig;
        sel.near_cap = pd.near_cap; sel.need_hint = hints.needs(); sel.near_thr = c->one_pass_select ? hints.select_depth() : nullptr;
        sel.tiles_x = (unsigned int)c->fc.tiles_x; sel.tile_rows = (unsigned int)c->fc.n_tile_rows;
        sel.grid = pd.select_grid; sel.at_rest = c->fc.start_hints == 1; sel.hint_radius = pd.hint_radius;
        launch_select(sel);
    }
    else if (pd.comp_sorts == 0) {
        SortArgs sort{};
        sort.s = ss; sort.knobs = &c->knobs; sort.n_tiles = m; sort.grids = {c->grid_big, c->grid_mid, c->grid_long};
        sort.lists = f.lists; sort.keys = f.keys; sort.status = f.d_st; sort.orig = c->orig; sort.fused_sort_max = c->fused_sort_max;
        launch_sort(sort);
    }
    HIP_TRY(c, f.mark(4, ss));
    return SPLAT_OK;
}

// Which lane composites?  Frames to one image stay on one lane (stream order is their write-after-write / in-out
// order, as always); a frame to another image takes the other lane when it may.  A frame that must not overlap
// (synchronous, statistics, overlap off) goes to lane 0 behind everything lane 1 still holds.
// Enqueues the waits the choice needs, enters the frame into the image table; *lane = 0 or 1.
int pick_lane(splat_ctx* c, const char* img_lo, const char* img_hi, bool may_overlap, int ring_entry, int* lane) {
    int li = 0;
    *lane = 0;
    if (!c->comp2) return SPLAT_OK;
    auto touches = [&](const splat_ctx::ImgRec& e) { return e.seq != 0 && img_lo < e.hi && e.lo < img_hi; };
    const splat_ctx::ImgRec* newest = nullptr;        // the most recent frame to (a part of) this image
    for (const auto& e : c->img_tab)
        if (touches(e) && (!newest || e.seq > newest->seq)) newest = &e;
    if (!may_overlap) li = 0;
    else if (newest) li = newest->lane;
    else li = c->lane[0].seq <= c->lane[1].seq ? 0 : 1;            // an image nobody holds: the lane idle for longer
    hipStream_t mine = li ? c->comp2 : c->stream;
    // Frames to this image on the OTHER lane come first.  (Ring events: when the ring wraps onto an entry the host
    // has waited for that frame -- harvest -- so a re-recorded event only ever stands for a LATER frame.)
    for (const auto& e : c->img_tab)
        if (touches(e) && e.lane != li && e.ring >= 0) HIP_TRY(c, hipStreamWaitEvent(mine, c->ring[e.ring].e[7], 0));
    if (!may_overlap && li == 0 && c->lane[1].seq != 0 && c->lane[1].ring >= 0)
        HIP_TRY(c, hipStreamWaitEvent(mine, c->ring[c->lane[1].ring].e[7], 0));
    // this frame's entry: the image's own one, else a free one, else the oldest -- whose frame this one then follows
    // (an image that drops out of the table must not be in flight any more)
    splat_ctx::ImgRec* slot = nullptr;
    for (auto& e : c->img_tab) if (e.seq != 0 && e.lo == img_lo && e.hi == img_hi) { slot = &e; break; }
    if (!slot) for (auto& e : c->img_tab) if (e.seq == 0) { slot = &e; break; }
    if (!slot) {
        for (auto& e : c->img_tab) if (!slot || e.seq < slot->seq) slot = &e;
        if (slot->ring >= 0) {      // (both lanes: whichever lane the forgotten image's next frame takes, it follows)
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ring[slot->ring].e[7], 0));
            HIP_TRY(c, hipStreamWaitEvent(c->comp2, c->ring[slot->ring].e[7], 0));
        }
    }
    slot->lo = img_lo; slot->hi = img_hi; slot->seq = c->lane_seq + 1; slot->ring = ring_entry; slot->lane = li;
    *lane = li;
    return SPLAT_OK;
}

// THE COMPOSITOR STAGE, on f.cs behind the ordering: the iteration buffer of a statistics frame, the launch, the late status, and
// the ring event that says the frame has ended.
int composite_frame(splat_ctx* c, const FrameLaunch& f, uint32_t* d_argb, bool want_iters) {
    Slot& s = *f.s;
    const splat_policy_decision& pd = f.pd;
    hipStream_t cs = f.cs;
    const unsigned int m = c->n_tiles;
    if (c->pre_wait) { HIP_TRY(c, hipStreamWaitEvent(cs, c->pre_wait, 0)); c->pre_wait = nullptr; }
    const bool retained = f.retain == SPLAT_RETAIN_RETAIN;      // (nothing in front of this compositor but the compositors before it, on this stream)
    if (c->pipeline && f.ss != cs && !retained) {
        HIP_TRY(c, hipEventRecord(s.ev_ready, f.ss));
        HIP_TRY(c, hipStreamWaitEvent(cs, s.ev_ready, 0));
    }
    // A retained frame's status is its own, from the values the writer's scan left: the compositor checks `overflow` and counts
    // its retries there (one 1-thread launch in front of it; the host copy is filled in enqueue_frame)
    if (retained) launch_status_set(cs, f.d_st, c->ret_set.status);
    HIP_TRY(c, f.mark(5, cs));
    uint2* iters = nullptr;
    c->iters_valid = false;
    if (want_iters) {       // statistics frame: every compositor wave leaves its iteration counts (plain stores)
        if (c->iters_alloc < m * 4u) {
            dfree(c->d_iters); c->iters_alloc = 0;
            HIP_TRY(c, dmalloc(c, &c->d_iters, sizeof(uint2) * (size_t)m * 4u));
            c->iters_alloc = m * 4u;
        }
        HIP_TRY(c, hipMemsetAsync(c->d_iters, 0, sizeof(uint2) * (size_t)m * 4u, cs));
        iters = c->d_iters;
        c->iters_valid = true;
    }
    CompositeArgs comp{};
    comp.s = cs; comp.knobs = &c->knobs; comp.n_tiles = m; comp.fc = c->fc; comp.recs = s.recs; comp.argb = d_argb; comp.status = f.d_st; comp.orig = c->orig;
    // (the writer's workgroups store every list they sort back to its region; a retained frame's read them all from there)
    comp.fused_sort_max = retained ? 0u : c->fused_sort_max; comp.iters = iters; comp.keep_keys = want_iters || f.retain == SPLAT_RETAIN_WRITER;
    // throughput-bound frames (many pairs per key of the longest list: C3 737, C5 3100) keep the one-record walk, the
    // others (C2 316, an eighth-of-a-frame slab 92, C1 36) take the paired one; measured crossover between 316 and 737
    comp.pair_walk = pd.pair_walk != 0;
    comp.libm_exp = (c->cfg.mode & SPLAT_MODE_LIBM_EXP) != 0; comp.clear_first = c->clear_first;
    // the frame's lists and key buffers, with what the compositor reads a meaning into: the second buffer only where it
    // orders the long lists itself, the selections' lengths only where launch_select ran
    comp.lists = f.lists; comp.lists.near_m = pd.near_cap ? s.near_m : nullptr;
    comp.keys = f.keys; comp.keys.keys2 = pd.comp_sorts != 0 ? s.keys2 : nullptr;
    if (retained) {
        // the long lists as the writer's ordering left them: its selections (near_m, the second key buffer), or in order in
        // their regions -- by its sort launches or its own workgroups -- which flavour 0 reads
        const bool near = c->ret_set.near_cap != 0u;
        comp.lists.near_m = near ? s.near_m : nullptr; comp.keys.keys2 = near ? s.keys2 : nullptr;
    }
    comp.hints = hint_table(c);
    // STAGING VERDICTS, kept from one retained frame to the next (CompArgs::stage_nv): the writer clears the counts -- once per
    // rest, and whatever ends a retained set leads to a new writer -- and the frames composited from its lists, which run
    // behind it on this stream, take and leave them.  Every other frame passes none.
    if (c->knobs.dbg_stage_cache != 0u && f.retain == SPLAT_RETAIN_WRITER) {
        const size_t waves = (size_t)c->m_alloc * 4u;
        if (!c->stage_nv || !c->stage_mask) {
            dfree(c->stage_nv); dfree(c->stage_mask);
            HIP_TRY(c, dmalloc(c, &c->stage_nv, sizeof(unsigned int) * 2u * waves));       // (the counts, then the proven starts)
            HIP_TRY(c, dmalloc(c, &c->stage_mask, sizeof(unsigned long long) * 32u * waves));
        }
        HIP_TRY(c, hipMemsetAsync(c->stage_nv, 0, sizeof(unsigned int) * 2u * waves, cs));
        c->ret_set.frames = 0;
    }
    if (retained && c->knobs.dbg_stage_cache != 0u && c->stage_nv && c->stage_mask) {
        comp.stage_nv = c->stage_nv; comp.stage_mask = c->stage_mask;
        // PROVEN STARTS (CompArgs::proven_start), behind the counts in one allocation: cleared with them by the set's writer,
        // written and read by the set's frames alone.  Exact modes only: a fast-mode frame depends on where its walks start.
        if (c->knobs.dbg_proven_starts != 0u && c->fc.close_width == 0.0f) comp.proven_start = c->proven_start();
        if (c->knobs.dbg_stage_cache == 2u && c->ret_set.frames >= 2u)
            HIP_TRY(c, hipMemsetAsync(c->stage_mask, 0, sizeof(unsigned long long) * 32u * (size_t)c->m_alloc * 4u, cs));
        c->ret_set.frames++;
    }
    comp.refine = c->fc.close_width == 0.0f ? pd.refine : 0u;      // (exact modes only: a fast-mode frame depends on where its walks start)
    launch_composite(comp);
    c->last_near = retained ? c->ret_set.near_cap != 0u : pd.near_cap != 0u;
    HIP_TRY(c, f.mark(6, cs));
    // the scan has already delivered this frame's status to h_status[r]; a statistics frame refreshes it with the late
    // counters (compositor retries, sort fallbacks)
    if (want_iters) HIP_TRY(c, hipMemcpyAsync(&c->h_status[f.r], f.d_st, sizeof(FrameStatus), hipMemcpyDeviceToHost, cs));
    HIP_TRY(c, hipEventRecord(f.ev->e[7], cs));
    return SPLAT_OK;
}

// RETAINED LISTS: this frame's decision (splat_retain_decide, include/splat_retain.h) from the camera's bytes, the binning
// epoch and the writer's status.  The frame behind a writer needs that writer's verdict: where its scan has not delivered
// it yet (a host that enqueues faster than the device renders), the host waits for the writer ONCE per rest -- the frames
// in flight drain, and what follows costs a compositor each.
int decide_retention(splat_ctx* c, const splat_camera* cam, int* action) {
    splat_retain_input in;
    std::memset(&in, 0, sizeof in);
    static_assert(sizeof(splat_camera) + 2 * sizeof(int32_t) <= sizeof in.cam, "the camera and the slab fit the decision's words");
    std::memcpy(in.cam, cam, sizeof(splat_camera));
    const int32_t slab[2] = {c->slab0, c->slab1};
    std::memcpy(reinterpret_cast<unsigned char*>(in.cam) + sizeof(splat_camera), slab, sizeof slab);
    in.epoch = c->bin_epoch; in.still_frames = c->pol.still_frames;
    // (a debug launch of the N longest tiles only would leave the other lists unsorted behind a writer)
    in.enabled = (c->retain_lists != 0 && c->knobs.dbg_ntiles == 0u) ? 1 : 0;
    in.overlap = c->overlap; in.one_pass = c->fc.bucket_cap ? 1 : 0;
    splat_retain_decision d;
    const int wr = c->ret_set.ring;
    for (int pass = 0; pass < 2; ++pass) {
        if (c->ret.writer == 1u && wr >= 0) {
            const volatile FrameStatus* hs = &c->h_status[wr];
            in.writer_arrived = hs->arrived; in.writer_overflow = hs->overflow; in.writer_redone = hs->redone;
        }
        if (splat_retain_decide(&c->ret, &in, &d) != 0) return fail(c, SPLAT_ERR_INVALID, "retention refused its input");
        // the writer's scan has not reported, and everything else says "retain" (d.wait_for_writer): wait for that frame -- its
        // ring event, the one event an untimed frame records -- and ask again with its status
        if (pass == 0 && d.wait_for_writer != 0 && wr >= 0 && c->ring[wr].used) {
            HIP_TRY(c, hipEventSynchronize(c->ring[wr].e[7]));
            continue;
        }
        break;
    }
    if (c->ret.writer == 1u && d.next.writer == 2u) {
        // established: the set's status is what the writer's scan delivered -- the late counters start from zero in every frame
        FrameStatus st = c->h_status[wr];
        st.n_fallback = 0; st.n_sort_fallback = 0; st.n_near_fallback = 0; st.n_probe_fail = 0; st.arrived = 1u;
        c->ret_set.status = st;
    }
    c->ret = d.next;
    *action = d.action;
    return SPLAT_OK;
}

// Enqueue one frame.  Blocks the host only when the event ring wraps onto a frame that is still running (32 frames
// behind), and once per rest for the writer of a retained set when its status has not arrived yet (decide_retention).
// `timed`: record the per-kernel timing events.  Every hipEventRecord is a barrier packet that
// drains its queue for a few microseconds -- nine of them per frame were ~25 us of bubbles in a
// 590 us frame -- so untimed frames (all but every `timing_every`-th of an asynchronous run) record
// only the one event that tells the host the frame's status has arrived.
// The stages: the frame's decisions (splat_policy_decide), bin_frame, order_frame, pick_lane, composite_frame.
int enqueue_frame(splat_ctx* c, const splat_camera* cam, uint32_t* d_argb, bool timed, bool want_iters = false, bool may_overlap = false, bool awaited = false) {
    FrameLaunch f{};
    const int r = c->ring_next;
    EvSet& ev = c->ring[r];
    f.r = r; f.ev = &ev; f.timed = timed;
    c->ring_next = (c->ring_next + 1) % EV_RING;
    harvest(c, r);
    std::memset(&c->h_status[r], 0, sizeof(FrameStatus));      // (this frame's scan fills it; until then it says nothing: see the peek below)
    // (slots and binning streams rotate with the frames that are BINNED: after retained frames binning resumes on the slot
    // behind the writer's, whose regions and cursors the frames before the writer prepared)
    int si = (int)(c->bin_idx % (uint64_t)slots_in_use(c));
    const uint64_t bin_no = c->bin_idx + 1;
    c->frame_idx++;
    Slot* sp = &c->slots[si];
    f.d_st = c->d_status_ring + r;       // (initialised by this frame's scan)
    // pipeline depth 1: everything on the caller's stream.  2: K1..K3 of frame N+1 on the bin stream
    // under the compositor of frame N.  3: K1 + scan of frame N+2 on the bin stream, K2 + K3 of
    // frame N+1 on the sort stream, compositor of frame N on the caller's stream -- the bin chain is
    // the longest of the three under contention, so splitting it raises the frame rate.
    f.bs = c->pipeline ? c->bin_stream : c->stream;
    // 6 (default): four slots, and the bin + sort chains of consecutive frames alternate between two streams, so
    // the chain of frame N+2 (a latency chain: K1 -> scan -> sort) runs beside the chain of frame N+1 and the
    // compositor of frame N.  With one chain at a time the frame time IS the chain's length under contention
    // (C3: 0.28 + 0.03 + 0.11 = 0.42 ms against a compositor of 0.37); two in flight leave the compositor as the
    // bound: C3 2241 -> 2334 fps, C1 17.4 k -> 19.2 k, C5 +1 %, C2 -1 %
    if (c->pipeline >= 6 && (bin_no & 1ull)) f.bs = c->sort_stream;
    f.ss = c->pipeline == 3 ? c->sort_stream : f.bs;     // (4, 5: three / four slots on two streams)
    // THE FRAME'S DECISIONS (include/splat_policy.h): everything below this call only launches what it says.
    {
        const splat_policy_knobs pk = policy_knobs_of(c);
        // (the slot the frame would be BINNED into: whether the frame is retained is decided behind the policy, from its still
        // count.  On a retained frame what the policy says about binning and ordering -- count_first, redo, near_cap,
        // comp_sorts, the launch sizes -- is not used: composite_frame takes the writer's ordering from ret_set.)
        const splat_policy_input pi = policy_input_of(c, *sp, r, awaited);
        if (splat_policy_decide(&pk, &c->pol, &pi, &f.pd) != 0) return fail(c, SPLAT_ERR_INVALID, "frame policy refused its input");
        c->pol = f.pd.next;
    }
    c->fc.start_hints = f.pd.start_hints_mode; c->fc.start_light = f.pd.start_light; c->fc.early_min = f.pd.early_min;
    // RETAINED LISTS (include/splat_retain.h): bin, bin as the writer, or composite from the writer's slot
    {
        int rc = decide_retention(c, cam, &f.retain);
        if (rc != SPLAT_OK) return rc;
    }
    if (f.retain == SPLAT_RETAIN_WRITER) { c->ret_set.slot = si; c->ret_set.ring = r; c->ret_set.near_cap = f.pd.near_cap; }
    // (the writer carries the per-kernel timing events whatever the sampling says: it is the one frame of a rest whose binning
    // and ordering exist to be timed -- splat_get_timing over a rest then still knows what a binned frame costs; its semantics
    // at rest are in include/splat_hip.h)
    if (f.retain == SPLAT_RETAIN_WRITER) { f.timed = true; timed = true; }
    if (f.retain == SPLAT_RETAIN_RETAIN) {
        si = c->ret_set.slot; sp = &c->slots[si];
        // the frame's status on the host is the writer's (the device copy: composite_frame), and it has arrived
        c->h_status[r] = c->ret_set.status;
        c->frames_retained++;
    } else c->bin_idx++;
    Slot& s = *sp;
    f.si = si; f.s = &s;
    // A frame the caller waits for, with nothing else in flight (the reference's loop: one synchronous frame per pose,
    // src/main.rs:69-78), has nothing to overlap with: its whole chain goes on the caller's stream, in order (pd.solo) -- no
    // event recorded on one stream and waited for on another between its binning and its compositor (two barrier packets and
    // a cross-queue hand-over: ~15 us of a 0.6-ms frame).
    if (f.pd.solo != 0) { f.bs = c->stream; f.ss = c->stream; }
    c->idle = false;
    // (two-pass binning: the second buffer mirrors the first)
    f.lists = {s.offsets, s.order, s.lens, s.cursor, c->fc.bucket_cap ? s.off2 : nullptr, s.near_m};
    f.keys = {s.keys, s.keys2, c->cap, (unsigned int)std::min<uint64_t>(c->cap2, 0xffffffffull)};
    int rc = SPLAT_OK;
    if (f.retain != SPLAT_RETAIN_RETAIN) {
        rc = bin_frame(c, f);
        if (rc == SPLAT_OK) rc = order_frame(c, f);
        if (rc != SPLAT_OK) return rc;
    }
    int li = 0;
    const char* const img_lo = reinterpret_cast<const char*>(d_argb);
    rc = pick_lane(c, img_lo, img_lo + (size_t)c->fc.W * (size_t)c->fc.H * 4u, may_overlap, r, &li);
    if (rc != SPLAT_OK) return rc;
    f.cs = li ? c->comp2 : c->stream;
    rc = composite_frame(c, f, d_argb, want_iters);
    if (rc != SPLAT_OK) return rc;
    s.free_ring = r;
    HIP_TRY(c, hipGetLastError());
    s.used = true;
    ev.used = true;
    ev.timed = timed;
    ev.retained = f.retain == SPLAT_RETAIN_RETAIN;
    c->last_ring = r;
    c->last_slot = si;
    c->lane[li].seq = ++c->lane_seq; c->lane[li].ring = r;
    c->last_lane = li;
    c->last_lists_in_memory = want_iters || c->fused_sort_max == 0 || f.retain != SPLAT_RETAIN_BIN;
    return SPLAT_OK;
}

// Wait for everything enqueued and harvest every frame's status.  Returns SPLAT_ERR_CAPACITY when at
// least one harvested frame was skipped on the device because it outgrew its storage (pair buffer, tile
// bucket, sort launch sizes): the storage / hints have then been grown for the next attempt.
// *last_skipped tells whether the MOST RECENT frame is among the skipped ones -- only that one may be
// redone by a synchronous caller (an older asynchronous frame that was lost must not make the current,
// complete frame blend a second time onto the in/out image).
int finish_frame(splat_ctx* c, bool* last_skipped = nullptr) {
    if (last_skipped) *last_skipped = false;
    int rc = sync_all(c);
    if (rc != SPLAT_OK) return rc;
    c->idle = true;                          // every stream of the context has drained
    if (c->last_ring >= 0) c->last = c->h_status[c->last_ring];
    if (last_skipped) *last_skipped = c->last_ring >= 0 && c->last.overflow != 0;
    for (int k = 0; k < EV_RING; ++k) harvest(c, k);
    const char* msg = nullptr;
    if (c->sort_grid_miss) {            // the hint has been refreshed from the frame that missed
        c->sort_grid_miss = false;
        msg = "more long tile lists than the sort launches covered; frame must be re-rendered";
    }
    if (c->bucket_overflow || c->layout_want) {
        // A tile's list outgrew the region it had been given (sized from a frame two back: the camera moved, or nothing
        // was known yet), or the regions did not fit the key buffer.  The slots' layouts are dropped -- the next frame
        // counts its pairs first (bootstrap, enqueue_frame) and gets regions that fit it -- and the buffer grows to what
        // the layout asked for.
        const bool overflowed = c->bucket_overflow;
        c->bucket_overflow = false;
        bump_epoch(c);
        for (Slot& sl : c->slots) sl.layout_valid = false;
        if (c->layout_want > c->cap) {
            const uint64_t asked = c->layout_want + c->layout_want / 4 + 1024, want = std::min<uint64_t>(asked, KEY_ENTRIES_MAX);
            const uint64_t bytes = (want + c->cap2) * 8ull * (uint64_t)slots_in_use(c);
            if (bytes > c->bucket_bytes || asked > KEY_ENTRIES_MAX) c->bucket_failed = true;    // no room: exactly sized lists instead
            else {
                rc = ensure_keys(c, want, c->cap2);
                if (rc == SPLAT_ERR_CAPACITY) { c->bucket_failed = true; rc = SPLAT_OK; }
                else if (rc != SPLAT_OK) return rc;
            }
        }
        c->layout_want = 0;
        if (overflowed) msg = "a tile outgrew its region of the key buffer; regions rebuilt, frame must be re-rendered";
    }
    if (c->overflow_want) {
        uint64_t want = (uint64_t)((double)c->overflow_want * 1.25) + 1024;
        c->overflow_want = 0;
        rc = ensure_keys(c, want, want);
        if (rc != SPLAT_OK) return rc;
        msg = "pair buffer overflowed; capacity grown, frame must be re-rendered";
    }
    if (c->keys2_want) {
        // the lists of more than 2048 keys asked for more room in the second key buffer than it has (a camera deep inside a
        // dense scene): a quarter more than they asked for
        const uint64_t want2 = std::min<uint64_t>(c->keys2_want + c->keys2_want / 4 + 1024, KEY_ENTRIES_MAX);
        c->keys2_want = 0;
        rc = ensure_keys(c, c->cap, want2);
        if (rc != SPLAT_OK) return rc;
        msg = "the long tile lists outgrew the second key buffer; buffer grown, frame must be re-rendered";
    }
    return msg ? fail(c, SPLAT_ERR_CAPACITY, msg) : SPLAT_OK;
}

// For the entry points that only wait (splat_sync, splat_get_*, ...): a skipped frame -- found now or left
// pending by a synchronous render that was itself complete -- is reported once.
int finish_and_report(splat_ctx* c) {
    int rc = finish_frame(c);
    c->frames_drop_reported = c->frames_dropped;
    if (rc == SPLAT_OK && c->deferred_drop) {
        c->deferred_drop = false;
        return fail(c, SPLAT_ERR_CAPACITY, "an earlier asynchronous frame was skipped on the device (storage has been grown); render it again");
    }
    if (rc == SPLAT_ERR_CAPACITY) c->deferred_drop = false;
    return rc;
}

// ... and for the ones that must quiesce the device on the way to something else (re-allocation, a count-only
// pass): a loss found here stays pending for the next report.
int finish_quiet(splat_ctx* c) {
    int rc = finish_frame(c);
    if (rc == SPLAT_ERR_CAPACITY) { c->deferred_drop = true; rc = SPLAT_OK; }
    return rc;
}

int slots_in_use(const splat_ctx* c) { return c->pipeline >= 5 ? 4 : (c->pipeline >= 3 ? 3 : (c->pipeline ? 2 : 1)); }

// Pick the binning path for a frame over m tiles and make sure its key storage exists.
int prepare_binning(splat_ctx* c, unsigned int m, FrameConst* fc) {
    const bool one_pass = one_pass_wanted(c, m);
    if (one_pass != c->last_one_pass || m != c->layout_m) {
        // another path or another tile grid: the counters hold the other path's state (cursors / zeros), the regions
        // describe another grid
        int rc = finish_quiet(c);
        if (rc != SPLAT_OK) return rc;
        for (Slot& sl : c->slots) {
            sl.layout_valid = false; sl.flip = 0;
            if (sl.counts) HIP_TRY(c, hipMemsetAsync(sl.counts, 0, sizeof(unsigned int) * (size_t)(m + 1), c->stream));
        }
        if (c->need_hint) HIP_TRY(c, hipMemsetAsync(c->need_hint, 0, hint_table(c).bytes(), c->stream));   // another grid: another tile under every index
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->last_one_pass = one_pass; c->layout_m = m;
        reset_policy(c);
    }
    fc->bucket_cap = 0;
    if (one_pass) {
        // key buffer: what the two-pass path would start with, unless a layout has asked for more (finish_frame grows it)
        // (always with the second buffer: a region may hold a list of any length, and a list beyond 16384 keys sorts as
        // runs merged through it -- fixed-stride buckets could cap the lists at what the buffers at hand could sort)
        // The buffer that does not fit (the byte budget, or the allocation itself fails: a device with less free memory than
        // the default assumes) is tried again at half the size, down to the 16 entries per Gaussian the two-pass path would
        // start with, before one-pass binning is given up for the scene.
        int rc = SPLAT_ERR_CAPACITY;
        for (uint64_t mult = default_region_multiplier(c); ; mult >>= 1) {
            const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(c->cap, region_capacity_for(c, mult)), KEY_ENTRIES_MAX);
            const uint64_t want2 = std::min<uint64_t>(std::max<uint64_t>(c->cap2, default_keys2_capacity(c)), KEY_ENTRIES_MAX);
            rc = ((want + want2) * 8ull * (uint64_t)slots_in_use(c) > c->bucket_bytes) ? SPLAT_ERR_CAPACITY : ensure_keys(c, want, want2);
            if (rc != SPLAT_ERR_CAPACITY || mult <= 16 || want <= c->cap) break;
            (void)hipGetLastError();
        }
        if (rc == SPLAT_OK) { fc->bucket_cap = (unsigned int)std::min<uint64_t>(c->cap, KEY_ENTRIES_MAX); return rc; }
        if (rc != SPLAT_ERR_CAPACITY) return rc;
        c->bucket_failed = true;                          // no room: exactly sized lists instead
        return prepare_binning(c, m, fc);
    }
    // two-pass binning: exactly sized lists, and a second buffer that mirrors the first (the merges and global-memory radix
    // passes of its longest lists address it through the lists' own offsets)
    const uint64_t want = std::max<uint64_t>(default_pair_capacity(c), c->cap);
    return ensure_keys(c, want, want);
}

void fill_stats(splat_ctx* c, splat_stats* st) {
    std::memset(st, 0, sizeof *st);
    st->n_gaussians = c->n;
    st->n_visible = c->last.n_visible;
    st->n_singular = c->last.n_singular;
    st->n_pairs = c->last.n_pairs;
    st->max_tile_len = c->last.max_tile_len;
    st->n_fallback = c->last.n_fallback;
    st->n_sort_fallback = c->last.n_sort_fallback;
    st->n_iter_scan = 0; st->n_iter_blend = 0;
    st->n_near_tiles = c->last.n_near_tiles; st->n_near_fallback = c->last.n_near_fallback;
    st->n_blocks_culled = 0;
    const unsigned int* binfo = c->last_slot >= 0 ? c->slots[c->last_slot].blockinfo : nullptr;
    if (binfo && c->last_ring >= 0 && (c->fc.cull_blocks || c->fc.bucket_cap)) {   // the frame has finished: sum its block words
        std::vector<unsigned int> f((c->n + 255) / 256);
        if (hipMemcpy(f.data(), binfo, f.size() * sizeof(unsigned int), hipMemcpyDeviceToHost) == hipSuccess) {
            uint64_t vis = 0, sing = 0;
            for (unsigned int v : f) {
                if (v & 0x80000000u) { st->n_blocks_culled++; continue; }
                vis += v & 0x1ffu; sing += (v >> 9) & 0x1ffu;
            }
            if (c->fc.bucket_cap) { st->n_visible = vis; st->n_singular = sing; }     // (two-pass binning counts on the device)
        }
    }
    // (one-pass binning counts the visible Gaussians in the block words summed above, not on the device)
    st->bytes_algorithmic = c->n * 148ull + st->n_visible * 48ull + c->last.n_pairs * 60ull +
                            (uint64_t)c->fc.W * (uint64_t)(c->fc.row_px1 - c->fc.row_px0) * 4ull;
    // flops_alg = sum over pixels of (its tile's list length) * 25, and the compositor's
    // measured (wave, record) iterations -- left by every wave of a frame rendered with a stats pointer
    if (c->last_slot >= 0 && c->last_ring >= 0 && c->n_tiles) {
        const Slot& sl = c->slots[c->last_slot];
        const size_t m = c->n_tiles;
        std::vector<unsigned int> len(m);
        if (c->last.overflow == 0 && hipMemcpy(len.data(), sl.lens, sizeof(unsigned int) * m, hipMemcpyDeviceToHost) == hipSuccess) {
            uint64_t f = 0;
            for (size_t t = 0; t < m; ++t) {
                const int tx = (int)(t % (size_t)c->fc.tiles_x), ty = (int)(t / (size_t)c->fc.tiles_x) + c->fc.tile_row0;
                const int pw = std::min(TILE, c->fc.W - tx * TILE), ph = std::min(TILE, std::min(c->fc.H, c->fc.row_px1) - ty * TILE);
                if (pw > 0 && ph > 0) f += (uint64_t)len[t] * (uint64_t)(pw * ph);
            }
            st->flops_algorithmic = f * 25ull;
        }
        if (c->iters_valid && c->d_iters) {
            std::vector<uint2> it(m * 4u);
            if (hipMemcpy(it.data(), c->d_iters, sizeof(uint2) * it.size(), hipMemcpyDeviceToHost) == hipSuccess)
            {
                if (c->knobs.dbg_starts) {
                    // (debug: the words are (list length, nearest keys the wave's walk needed) -- how much of every list had to
                    // be in order at all, by list length class)
                    const unsigned int edges[6] = {0u, 768u, 2048u, 8192u, 16384u, 0xffffffffu};
                    for (int cls = 0; cls < 5; ++cls) {
                        uint64_t tiles = 0, keys = 0, need = 0, need2k = 0, full = 0;
                        for (size_t t = 0; t < m; ++t) {
                            const unsigned int len = std::max(std::max(it[4 * t].x, it[4 * t + 1].x), std::max(it[4 * t + 2].x, it[4 * t + 3].x));
                            if (len == 0 || len <= edges[cls] || len > edges[cls + 1]) continue;
                            unsigned int nd = 0;
                            for (int w = 0; w < 4; ++w) nd = std::max(nd, it[4 * t + w].y);
                            ++tiles; keys += len; need += nd; need2k += nd <= 2048u ? 1u : 0u; full += nd >= len ? 1u : 0u;
                        }
                        std::fprintf(stderr, "lists of %u < len <= %u keys: %llu tiles, %llu keys, deepest wave start needs %llu of them (%.1f %%); "
                                     "%llu tiles need <= 2048 keys, %llu need the whole list\n", edges[cls], edges[cls + 1],
                                     (unsigned long long)tiles, (unsigned long long)keys, (unsigned long long)need, keys ? 100.0 * need / keys : 0.0,
                                     (unsigned long long)need2k, (unsigned long long)full);
                    }
                } else
                for (const uint2& v : it) { st->n_iter_scan += v.x; st->n_iter_blend += v.y; }
                if (std::getenv("SPLAT_DBG_IMBALANCE")) {      // how much of a tile's four wave slots its slowest wave leaves idle
                    double sum = 0, held = 0;
                    for (size_t t = 0; t < m; ++t) {
                        double mx = 0;
                        for (int w = 0; w < 4; ++w) { const double cst = 14.0 * it[4 * t + w].x + 50.0 * it[4 * t + w].y + 300.0; sum += cst; mx = std::max(mx, cst); }
                        held += 4.0 * mx;
                    }
                    std::fprintf(stderr, "compositor wave imbalance: sum of wave costs / (4 x slowest wave per tile) = %.3f\n", held > 0 ? sum / held : 1.0);
                    // ... and what the early-out scan bought: waves that scanned, split by whether the exact walk then took
                    // about as many steps as the scan (it found its start) or at least twice as many (it gave up half way)
                    uint64_t sc_ok = 0, bl_ok = 0, sc_no = 0, bl_no = 0, w_ok = 0, w_no = 0, bl_none = 0;
                    for (const uint2& v : it) {
                        if (v.x == 0) { bl_none += v.y; continue; }
                        if ((uint64_t)v.y * 10u >= (uint64_t)v.x * 18u) { sc_no += v.x; bl_no += v.y; ++w_no; } else { sc_ok += v.x; bl_ok += v.y; ++w_ok; }
                    }
                    std::fprintf(stderr, "early-out scan: %llu waves found a start (scan %llu, blend %llu steps), %llu did not (scan %llu, blend %llu); waves without a scan: blend %llu\n",
                                 (unsigned long long)w_ok, (unsigned long long)sc_ok, (unsigned long long)bl_ok, (unsigned long long)w_no, (unsigned long long)sc_no,
                                 (unsigned long long)bl_no, (unsigned long long)bl_none);
                }
            }
        }
    }
    float t[N_TIMES] = {0};
    if (c->last_ring >= 0 && c->ring[c->last_ring].timed) ev_times(c->ring[c->last_ring], t);   // events stay valid after harvest
    st->ms_preprocess = t[0]; st->ms_scan = t[1]; st->ms_emit = t[2]; st->ms_sort = t[3]; st->ms_composite = t[4];
    st->ms_total = t[0] + t[1] + t[2] + t[3] + t[4];
}

}  // namespace

namespace {
// One option, validated and stored (include/splat_hip.h SPLAT_OPT_*).  The caller has quiesced the context where that
// matters.  false: unknown option or value out of range.
// dry: validate only (splat_set_option checks the value before it touches anything, pinned options included)
bool store_option(splat_ctx* c, int opt, double v, bool dry = false) {
    if (!(v == v)) return false;
#define SPLAT_DRY_ if (dry) return true
    switch (opt) {
        case SPLAT_OPT_PIPELINE_DEPTH: {
            if (v < 1.0 || v > 6.0) return false;
            SPLAT_DRY_;
            const int p = (int)v <= 1 ? 0 : (int)v;
            if (p != c->pipeline) {
                // another number of frame slots: the key buffers exist per slot in use and are made again by the next frame
                for (Slot& sl : c->slots) { dfree(sl.keys); dfree(sl.keys2); sl.layout_valid = false; sl.flip = 0; sl.used = false; sl.free_ring = -1; }
                c->cap = 0; c->cap2 = 0; c->frame_idx = 0; c->bin_idx = 0;
                c->pipeline = p;
                // One stream for everything has no compositor lanes: the lane state goes as splat_set_frame_overlap(1) leaves it
                // (unless the operator pinned the overlap from the environment: then only the second lane's stream is dropped, and
                // the lanes come back -- ensure_lane, at the next frame that may overlap -- when the depth goes up again).  A depth
                // raised again does NOT restore an overlap of 2 set from code: set it again.
                if (p == 0) {
                    c->comp2 = nullptr;
                    if (!(c->env_pinned & (1u << SPLAT_OPT_FRAME_OVERLAP))) c->overlap = 1;
                    c->lane[0] = splat_ctx::Lane{}; c->lane[1] = splat_ctx::Lane{};
                    for (auto& e : c->img_tab) e = splat_ctx::ImgRec{};
                    c->last_lane = 0;
                }
            }
            return true;
        }
        case SPLAT_OPT_FUSED_SORT_MAX: if (v < 0.0 || v > 2048.0) return false; SPLAT_DRY_; c->fused_sort_max = (unsigned int)v; return true;
        case SPLAT_OPT_REGION_SPARE: if (v < 1.0) return false; SPLAT_DRY_; c->region_spare = (float)v; return true;
        case SPLAT_OPT_EARLY_OUT_EPS: if (v < 0.0 || v > 1.0) return false; SPLAT_DRY_; c->early_eps = (float)v; return true;
        case SPLAT_OPT_EARLY_OUT_MIN_LIST: if (v < 0.0 || v > 1e9) return false; SPLAT_DRY_; c->early_min = (int)v; return true;
        case SPLAT_OPT_EARLY_OUT_SCAN_EIGHTHS: if (v < 1.0 || v > 8.0) return false; SPLAT_DRY_; c->early_scan8 = (int)v; return true;
        case SPLAT_OPT_SORT_IN_COMPOSITOR: if (v < -1.0 || v > 1.0) return false; SPLAT_DRY_; c->sort_in_comp = v < 0.0 ? -1 : (v != 0.0 ? 1 : 0); return true;
        case SPLAT_OPT_PAIR_WALK: if (v < -1.0 || v > 1.0) return false; SPLAT_DRY_; c->pair_mode = v < 0.0 ? -1 : (v != 0.0 ? 1 : 0); return true;
        case SPLAT_OPT_TIMING_EVERY: if (v < 1.0 || v > 1e9) return false; SPLAT_DRY_; c->timing_every = (int)v; return true;
        case SPLAT_OPT_BLOCK_CULLING: if (v != 0.0 && v != 1.0) return false; SPLAT_DRY_; c->cull_blocks = v != 0.0; return true;
        case SPLAT_OPT_ONE_PASS_BINNING: if (v != 0.0 && v != 1.0) return false; SPLAT_DRY_; c->use_buckets = v != 0.0; return true;
        case SPLAT_OPT_KEY_BUFFER_BYTES: if (v < 0.0 || v > 1.8e19) return false; SPLAT_DRY_; c->bucket_bytes = (uint64_t)v; c->bucket_failed = false; return true;
        case SPLAT_OPT_FAST_CLOSE_WIDTH: if (v != 1.0 && v != 2.0) return false; SPLAT_DRY_; c->fast_width = (float)v; return true;
        case SPLAT_OPT_PRIORITY_LIST_LEN: if (v < 1.0 || v > 1073741823.0) return false; SPLAT_DRY_; c->prio_len = (int)v; return true;
        case SPLAT_OPT_FRAME_OVERLAP: if (v != 1.0 && v != 2.0) return false; SPLAT_DRY_; c->overlap = (int)v; return true;    // (lanes: splat_set_option / splat_create make them)
        case SPLAT_OPT_NEAR_SELECT_KEYS: if (v != 0.0 && (v < 64.0 || v > 2048.0)) return false; SPLAT_DRY_; c->near_cap = (unsigned int)v; return true;
        case SPLAT_OPT_OVERFLOW_REDO: if (v != 0.0 && v != 1.0 && v != 2.0) return false; SPLAT_DRY_; c->overflow_redo = (int)v; return true;
        case SPLAT_OPT_START_HINTS: if (v != 0.0 && v != 1.0 && v != 2.0) return false; SPLAT_DRY_; c->start_hints = (int)v; return true;
        case SPLAT_OPT_HOST_ZERO_COPY: if (v != 0.0 && v != 1.0) return false; SPLAT_DRY_; c->host_zero_copy = (int)v; return true;
        case SPLAT_OPT_COUNT_FIRST: if (v != 0.0 && v != 1.0 && v != 2.0) return false; SPLAT_DRY_; c->count_first = (int)v; return true;
        case SPLAT_OPT_KEYS_PER_GAUSSIAN: if (v != 0.0 && (v < 4.0 || v > 256.0)) return false; SPLAT_DRY_; c->keys_per_gaussian = (unsigned int)v; return true;
        case SPLAT_OPT_LARGE_SPLAT_TILES: if (v < -1.0 || v > 1048576.0 || v != std::floor(v)) return false; SPLAT_DRY_; c->large_tiles = (int)v; return true;
        case SPLAT_OPT_LARGE_LIST_MIN: if (v < -1.0 || v > 1e9 || v != std::floor(v)) return false; SPLAT_DRY_; c->large_list_min = (int)v; return true;
        case SPLAT_OPT_START_REFINE: if (v != 0.0 && v != 1.0) return false; SPLAT_DRY_; c->start_refine = (int)v; return true;
        case SPLAT_OPT_RETAIN_LISTS: if (v != 0.0 && v != 1.0) return false; SPLAT_DRY_; c->retain_lists = (int)v; return true;
        default: return false;
    }
#undef SPLAT_DRY_
}
bool load_option(const splat_ctx* c, int opt, double* v) {
    switch (opt) {
        case SPLAT_OPT_PIPELINE_DEPTH: *v = c->pipeline ? c->pipeline : 1; return true;
        case SPLAT_OPT_FUSED_SORT_MAX: *v = c->fused_sort_max; return true;
        case SPLAT_OPT_REGION_SPARE: *v = c->region_spare; return true;
        case SPLAT_OPT_EARLY_OUT_EPS: *v = c->early_eps; return true;
        case SPLAT_OPT_EARLY_OUT_MIN_LIST: *v = c->early_min; return true;
        case SPLAT_OPT_EARLY_OUT_SCAN_EIGHTHS: *v = c->early_scan8; return true;
        case SPLAT_OPT_SORT_IN_COMPOSITOR: *v = c->sort_in_comp; return true;
        case SPLAT_OPT_PAIR_WALK: *v = c->pair_mode; return true;
        case SPLAT_OPT_TIMING_EVERY: *v = c->timing_every; return true;
        case SPLAT_OPT_BLOCK_CULLING: *v = c->cull_blocks ? 1 : 0; return true;
        case SPLAT_OPT_ONE_PASS_BINNING: *v = c->use_buckets ? 1 : 0; return true;
        case SPLAT_OPT_KEY_BUFFER_BYTES: *v = (double)c->bucket_bytes; return true;
        case SPLAT_OPT_FAST_CLOSE_WIDTH: *v = c->fast_width; return true;
        case SPLAT_OPT_PRIORITY_LIST_LEN: *v = c->prio_len; return true;
        case SPLAT_OPT_FRAME_OVERLAP: *v = c->overlap; return true;
        case SPLAT_OPT_NEAR_SELECT_KEYS: *v = c->near_cap; return true;
        case SPLAT_OPT_OVERFLOW_REDO: *v = c->overflow_redo; return true;
        case SPLAT_OPT_START_HINTS: *v = c->start_hints; return true;
        case SPLAT_OPT_HOST_ZERO_COPY: *v = c->host_zero_copy; return true;
        case SPLAT_OPT_KEYS_PER_GAUSSIAN: *v = c->keys_per_gaussian; return true;
        case SPLAT_OPT_COUNT_FIRST: *v = c->count_first; return true;
        case SPLAT_OPT_LARGE_SPLAT_TILES: *v = c->large_tiles; return true;
        case SPLAT_OPT_LARGE_LIST_MIN: *v = c->large_list_min; return true;
        case SPLAT_OPT_START_REFINE: *v = c->start_refine; return true;
        case SPLAT_OPT_RETAIN_LISTS: *v = c->retain_lists; return true;
        default: return false;
    }
}
// The environment's say, at splat_create: the variable of an option, when set, stores it (clamped into the option's
// range as the variables always were) and pins it.
void option_from_env(splat_ctx* c, int opt, const char* name, double lo, double hi) {
    const char* e = std::getenv(name);
    if (!e || !*e) return;
    double v = std::atof(e);
    if (!(v == v)) return;
    v = std::min(hi, std::max(lo, v));
    if (store_option(c, opt, v)) c->env_pinned |= 1u << opt;
}
}  // namespace

namespace splat {
// wait for everything this context has enqueued; a frame found skipped stays pending for the next splat_sync to report
int ctx_quiesce(splat_ctx* c) { return finish_quiet(c); }
}  // namespace splat

extern "C" {

uint32_t splat_abi_version(void) { return SPLAT_ABI_VERSION; }
uint64_t splat_stats_size(void) { return sizeof(splat_stats); }

void splat_default_config(splat_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->device = 0;
    cfg->mode = SPLAT_MODE_EXACT;
    cfg->y_up = 1;          // pinned: notes/screenshot.png has the orientation of the notebook render
    cfg->sample_half = 1;   // euc samples pixel centres (unpinned)
    cfg->zclip = 1; cfg->zmin = 0.0f; cfg->zmax = 1.0f;   // euc CoordinateMode::VULKAN default (unpinned)
    cfg->pair_capacity = 0;
}

int splat_create(const splat_config* cfg, splat_ctx** out) {
    if (!out) return fail(nullptr, SPLAT_ERR_INVALID, "out is NULL");
    *out = nullptr;
    splat_config def;
    splat_default_config(&def);
    if (!cfg) cfg = &def;
    if (cfg->mode & ~(SPLAT_MODE_CORRECTED_PROJECTION | SPLAT_MODE_LIBM_EXP | SPLAT_MODE_FAST))
        return fail(nullptr, SPLAT_ERR_INVALID, "unknown mode");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SPLAT_ERR_HIP, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, SPLAT_ERR_INVALID, "device ordinal out of range");
    splat_ctx* c = new (std::nothrow) splat_ctx();
    if (!c) return fail(nullptr, SPLAT_ERR_INVALID, "out of host memory");
    c->cfg = *cfg;
    if (cfg->mode & SPLAT_MODE_FAST) {
        c->early_eps = 2e-3f;      // hi - lo <= 2 needs a contraction of ~1/128, not of ~1e-5 ...
        c->early_min = 384;        // ... which lists of a few hundred keys reach too (C3: 2960 -> 3125 frames/s; exact mode: 768 is best)
    }
    // the options a host reaches through splat_set_option; their environment variables pin them (include/splat_hip.h)
    option_from_env(c, SPLAT_OPT_SORT_IN_COMPOSITOR, "SPLAT_SORT_IN_COMP", -1, 1);
    if (const char* e0 = std::getenv("SPLAT_FAST_WIDTH")) { c->fast_width = std::atoi(e0) <= 1 ? 1.0f : 2.0f; c->env_pinned |= 1u << SPLAT_OPT_FAST_CLOSE_WIDTH; }
    option_from_env(c, SPLAT_OPT_EARLY_OUT_EPS, "SPLAT_EARLY_EPS", 0, 1);
    option_from_env(c, SPLAT_OPT_EARLY_OUT_MIN_LIST, "SPLAT_EARLY_MIN", 0, 1e9);
    option_from_env(c, SPLAT_OPT_EARLY_OUT_SCAN_EIGHTHS, "SPLAT_EARLY_SCAN8", 1, 8);
    option_from_env(c, SPLAT_OPT_PRIORITY_LIST_LEN, "SPLAT_PRIO_LEN", 1, 1073741823.0);
    option_from_env(c, SPLAT_OPT_FRAME_OVERLAP, "SPLAT_FRAME_OVERLAP", 1, 2);
    option_from_env(c, SPLAT_OPT_PIPELINE_DEPTH, "SPLAT_PIPELINE", 1, 6);
    option_from_env(c, SPLAT_OPT_TIMING_EVERY, "SPLAT_TIMING_EVERY", 1, 1e9);
    option_from_env(c, SPLAT_OPT_FUSED_SORT_MAX, "SPLAT_FUSED_SORT", 0, 2048);
    if (const char* e5 = std::getenv("SPLAT_BUCKETS")) { c->use_buckets = std::atoi(e5) != 0; c->env_pinned |= 1u << SPLAT_OPT_ONE_PASS_BINNING; }
    if (const char* e7 = std::getenv("SPLAT_CULL")) { c->cull_blocks = std::atoi(e7) != 0; c->env_pinned |= 1u << SPLAT_OPT_BLOCK_CULLING; }
    if (const char* e8 = std::getenv("SPLAT_DBG_TIGHT_GRIDS")) c->tight_grids = std::atoi(e8) != 0;
    option_from_env(c, SPLAT_OPT_PAIR_WALK, "SPLAT_PAIR_BLEND", -1, 1);
    if (const char* e6 = std::getenv("SPLAT_BUCKET_BYTES")) { c->bucket_bytes = std::strtoull(e6, nullptr, 10); c->env_pinned |= 1u << SPLAT_OPT_KEY_BUFFER_BYTES; }
    option_from_env(c, SPLAT_OPT_REGION_SPARE, "SPLAT_REGION_SPARE", 1, 1e9);
    if (const char* er = std::getenv("SPLAT_OVERFLOW_REDO")) { c->overflow_redo = std::min(2, std::max(0, std::atoi(er))); c->env_pinned |= 1u << SPLAT_OPT_OVERFLOW_REDO; }
    if (const char* en = std::getenv("SPLAT_NEAR_KEYS")) {
        const int v = std::atoi(en);
        c->near_cap = v <= 0 ? 0u : (unsigned int)std::min(2048, std::max(64, v));
        c->env_pinned |= 1u << SPLAT_OPT_NEAR_SELECT_KEYS;
    }
    option_from_env(c, SPLAT_OPT_HOST_ZERO_COPY, "SPLAT_HOST_ZERO_COPY", 0, 1);
    option_from_env(c, SPLAT_OPT_COUNT_FIRST, "SPLAT_COUNT_FIRST", 0, 2);
    if (const char* kg = std::getenv("SPLAT_KEYS_PER_GAUSSIAN")) {
        const int v = std::atoi(kg);
        c->keys_per_gaussian = v <= 0 ? 0u : (unsigned int)std::min(256, std::max(4, v));
        c->env_pinned |= 1u << SPLAT_OPT_KEYS_PER_GAUSSIAN;
    }
    option_from_env(c, SPLAT_OPT_LARGE_SPLAT_TILES, "SPLAT_LARGE_TILES", -1, 1048576);
    option_from_env(c, SPLAT_OPT_LARGE_LIST_MIN, "SPLAT_LARGE_LIST_MIN", -1, 1e9);
    option_from_env(c, SPLAT_OPT_START_REFINE, "SPLAT_START_REFINE", 0, 1);
    option_from_env(c, SPLAT_OPT_RETAIN_LISTS, "SPLAT_RETAIN", 0, 1);
    if (const char* lm = std::getenv("SPLAT_LAYOUT_MOTION")) c->layout_motion = std::atoi(lm) != 0 ? 1 : 0;
    if (const char* k1 = std::getenv("SPLAT_SORT_RADIX_MIN")) c->knobs.sort_radix_min = (unsigned int)std::max(0, std::atoi(k1));
    if (const char* k2 = std::getenv("SPLAT_SCAN_THREADS")) c->knobs.scan_threads = std::atoi(k2);
    if (const char* k3 = std::getenv("SPLAT_DBG_NTILES")) c->knobs.dbg_ntiles = (unsigned int)std::max(0, std::atoi(k3));
    if (const char* k8 = std::getenv("SPLAT_DBG_SELECT_STRIDE")) c->knobs.dbg_select_stride = (unsigned int)std::max(0, std::atoi(k8));
    if (const char* k10 = std::getenv("SPLAT_START_HINTS")) { c->start_hints = std::min(2, std::max(0, std::atoi(k10))); c->env_pinned |= 1u << SPLAT_OPT_START_HINTS; }
    if (const char* k7 = std::getenv("SPLAT_DBG_ONE_PASS_SELECT")) c->one_pass_select = std::atoi(k7) != 0;
    if (const char* k11 = std::getenv("SPLAT_DBG_KEYS2_ENTRIES")) c->knobs.dbg_keys2_entries = std::strtoull(k11, nullptr, 10);
    if (const char* k9 = std::getenv("SPLAT_DBG_HINT_RADIUS")) c->knobs.dbg_hint_radius = std::atoi(k9);
    if (const char* k12 = std::getenv("SPLAT_DBG_SELECT_BLIND")) c->knobs.dbg_select_blind = std::atoi(k12) != 0 ? 1u : 0u;
    if (const char* k15 = std::getenv("SPLAT_DBG_PROVEN_STARTS")) c->knobs.dbg_proven_starts = (unsigned int)std::min(2, std::max(0, std::atoi(k15)));
    if (const char* k14 = std::getenv("SPLAT_DBG_BRACKET_COUNT")) c->knobs.dbg_bracket_count = std::atoi(k14) != 0 ? 1u : 0u;
    if (const char* k13 = std::getenv("SPLAT_DBG_STAGE_CACHE")) c->knobs.dbg_stage_cache = (unsigned int)std::min(2, std::max(0, std::atoi(k13)));
    if (const char* k5 = std::getenv("SPLAT_DBG_STARTS")) c->knobs.dbg_starts = std::atoi(k5) != 0 ? 1u : 0u;
    if (const char* k4 = std::getenv("SPLAT_COMP_LDS_PAD")) c->knobs.comp_lds_pad = (unsigned int)std::max(0, std::atoi(k4));
    if (const char* k1p = std::getenv("SPLAT_K1_LDS_PAD")) c->knobs.k1_lds_pad = (unsigned int)std::min(48 * 1024, std::max(0, std::atoi(k1p)));
    auto bail = [&](const char* what, hipError_t err) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        splat_destroy(c);
        return SPLAT_ERR_HIP;
    };
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = init_device_kernels()) != hipSuccess) return bail("hipFuncSetAttribute", e);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    c->own_stream = true;
    {   // The binning streams are separate hardware queues from the caller's stream.  With ONE chain in flight
        // (SPLAT_PIPELINE <= 5) they get the highest priority: the chain is the frame's critical path and its
        // short kernels should not queue behind a frame-long compositor (normal priority: 2174 -> 1969 fps).
        // With TWO chains in flight (6, the default) the compositor is the critical path and the chains run at
        // its priority (2349 -> 2384 fps on C3, C5 +1 %, C2 unchanged).
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        int prio = c->pipeline >= 6 ? (lo + hi) / 2 : hi;
        if (const char* ep = std::getenv("SPLAT_BIN_PRIO")) prio = std::atoi(ep) > 0 ? hi : (std::atoi(ep) < 0 ? lo : (lo + hi) / 2);
        if ((e = hipStreamCreateWithPriority(&c->bin_stream, hipStreamNonBlocking, prio)) != hipSuccess) return bail("hipStreamCreate", e);
        if ((e = hipStreamCreateWithPriority(&c->sort_stream, hipStreamNonBlocking, prio)) != hipSuccess) return bail("hipStreamCreate", e);
    }
    if (c->overlap >= 2 && c->pipeline) { if ((e = ensure_copy_stream(c)) != hipSuccess) return bail("hipStreamCreate", e); c->comp2 = c->copy_stream; }
    for (Slot& s : c->slots) {
        if ((e = dmalloc(c, &s.d_status, sizeof(FrameStatus))) != hipSuccess) return bail("hipMalloc(status)", e);
        if ((e = fill_now(s.d_status, 0, sizeof(FrameStatus))) != hipSuccess) return bail("fill_now(status)", e);
        if ((e = hipEventCreateWithFlags(&s.ev_ready, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&s.ev_binned, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", e);
    }
    if ((e = dmalloc(c, &c->d_status_ring, sizeof(FrameStatus) * EV_RING)) != hipSuccess) return bail("hipMalloc(status ring)", e);
    if ((e = fill_now(c->d_status_ring, 0, sizeof(FrameStatus) * EV_RING)) != hipSuccess) return bail("fill_now(status ring)", e);
    if ((e = hipHostMalloc(&c->h_status, sizeof(FrameStatus) * EV_RING, hipHostMallocCoherent)) != hipSuccess) return bail("hipHostMalloc(status)", e);
    std::memset(c->h_status, 0, sizeof(FrameStatus) * EV_RING);
    for (auto& s : c->ring)
        for (auto& ev : s.e)
            if ((e = hipEventCreate(&ev)) != hipSuccess) return bail("hipEventCreate", e);
    *out = c;
    return SPLAT_OK;
}

void splat_destroy(splat_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->bin_stream) (void)hipStreamSynchronize(c->bin_stream);
    if (c->sort_stream) (void)hipStreamSynchronize(c->sort_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);      // lane 1: compositors and gathers that use the buffers / the communicator released below
    if (c->comm) { comm_release(c->comm); c->comm = nullptr; }
    free_scene(c);
    dfree(c->zero_layout); dfree(c->need_hint); dfree(c->stage_nv); dfree(c->stage_mask);
    for (Slot& s : c->slots) {
        dfree(s.counts); dfree(s.offsets); dfree(s.cursor); dfree(s.order); dfree(s.lens); dfree(s.counts_b); dfree(s.lay_a); dfree(s.lay_b);
        dfree(s.near_m); dfree(s.redo_layout); dfree(s.redo_cursors); dfree(s.off2);
        dfree(s.keys); dfree(s.keys2); dfree(s.d_status);
        if (s.ev_ready) (void)hipEventDestroy(s.ev_ready);
        if (s.ev_binned) (void)hipEventDestroy(s.ev_binned);
    }
    dfree(c->d_img); dfree(c->d_iters);
    for (int k = 0; k < splat_ctx::S_IMGS; ++k) {
        dfree(c->s_img[k]);
        if (c->s_rendered[k]) (void)hipEventDestroy(c->s_rendered[k]);
        if (c->s_copied[k]) (void)hipEventDestroy(c->s_copied[k]);
    }
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    if (c->h_status) (void)hipHostFree(c->h_status);
    dfree(c->d_status_ring);
    for (auto& s : c->ring)
        for (auto& ev : s.e)
            if (ev) (void)hipEventDestroy(ev);
    if (c->bin_stream) (void)hipStreamDestroy(c->bin_stream);
    if (c->sort_stream) (void)hipStreamDestroy(c->sort_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    {   // (nothing of this context may stay in the allocation table: an entry outliving it would be a dangling owner)
        std::lock_guard<std::mutex> g(g_ledger_mu);
        for (auto it = g_ledger.begin(); it != g_ledger.end();) it = (it->second.first == c) ? g_ledger.erase(it) : std::next(it);
    }
    delete c;
}

const char* splat_last_error(const splat_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

void* splat_stream(splat_ctx* c) { return c ? (void*)c->stream : nullptr; }

int splat_set_frame_overlap(splat_ctx* c, int32_t n) {
    if (!c) return SPLAT_ERR_INVALID;
    if (n < 1 || n > 2) return fail(c, SPLAT_ERR_INVALID, "frame overlap is 1 or 2");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = finish_quiet(c);
    if (rc != SPLAT_OK) return rc;
    bump_epoch(c);
    c->overlap = n;
    if (n >= 2) return ensure_lane(c);
    c->comp2 = nullptr;                    // (the stream stays: it is the copy stream)
    c->lane[0] = splat_ctx::Lane{}; c->lane[1] = splat_ctx::Lane{};
    for (auto& e : c->img_tab) e = splat_ctx::ImgRec{};
    c->last_lane = 0;
    return SPLAT_OK;
}

int splat_set_option(splat_ctx* c, int32_t option, double value) {
    if (!c) return SPLAT_ERR_INVALID;
    if (option < 1 || option > 31) return fail(c, SPLAT_ERR_INVALID, "unknown option");
    double cur;
    if (!load_option(c, option, &cur)) return fail(c, SPLAT_ERR_INVALID, "unknown option");
    // the value is checked before anything else happens: an invalid one is an error whether or not the option is pinned, and
    // leaves the context as it was
    if (option == SPLAT_OPT_FRAME_OVERLAP ? (value != 1.0 && value != 2.0) : !store_option(c, option, value, true))
        return fail(c, SPLAT_ERR_INVALID, "option value out of range");
    if (c->env_pinned & (1u << option)) return SPLAT_OK;      // the operator's environment variable stays in force
    reset_policy(c);      // (the next frames scan for their walks' starts again, nothing stays armed: thresholds may have changed;
                          // and a retained set ends -- reset_policy bumps the binning epoch -- whichever option it is: none is exempt)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = finish_quiet(c);
    if (rc != SPLAT_OK) return rc;
    if (option == SPLAT_OPT_FRAME_OVERLAP) return splat_set_frame_overlap(c, (int32_t)value);
    if (option == SPLAT_OPT_KEYS_PER_GAUSSIAN) {
        // another key buffer size: the buffers are made again by the next frame (prepare_binning), the regions with them
        for (Slot& sl : c->slots) { dfree(sl.keys); dfree(sl.keys2); sl.layout_valid = false; sl.flip = 0; }
        c->cap = 0; c->cap2 = 0; c->bucket_failed = false;
    }
    if (!store_option(c, option, value)) return fail(c, SPLAT_ERR_INVALID, "option value out of range");
    // (another selection size: what the tiles' walks needed under the old one is forgotten)
    if (option == SPLAT_OPT_NEAR_SELECT_KEYS && c->need_hint && c->m_alloc)
        HIP_TRY(c, fill_now(c->need_hint, 0, hint_table(c).bytes()));
    // (the large list switched on with a scene in place: its buffers exist from now on -- splat_upload_scene makes them otherwise)
    if (option == SPLAT_OPT_LARGE_SPLAT_TILES && c->large_tiles >= 0 && c->n != 0)
        for (Slot& sl : c->slots)
            if (!sl.large_list) {
                HIP_TRY(c, dmalloc(c, &sl.large_list, sizeof(uint4) * c->n));
                if (!sl.large_count) HIP_TRY(c, dmalloc(c, &sl.large_count, sizeof(unsigned int) * 4));
                HIP_TRY(c, fill_now(sl.large_count, 0, sizeof(unsigned int) * 4));
            }
    return SPLAT_OK;
}

int splat_get_option(const splat_ctx* c, int32_t option, double* value) {
    if (!c || !value) return SPLAT_ERR_INVALID;
    return load_option(c, option, value) ? SPLAT_OK : SPLAT_ERR_INVALID;
}

int splat_set_stream(splat_ctx* c, void* stream) {
    if (!c) return SPLAT_ERR_INVALID;
    int rc = finish_quiet(c);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
    return rc;
}

}  // extern "C"

// ---- The scheduler's side of the seam to splat_scene.hip (splat_context.h)
namespace splat {
// The scene is being replaced: its frames end, and nothing of them is left to redo or to report.
int end_frames_for_upload(splat_ctx* c) {
    bump_epoch(c);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    (void)finish_frame(c);          // (frames of the scene being replaced: nothing left to redo)
    c->deferred_drop = false; c->frames_drop_reported = c->frames_dropped;
    return sync_all(c);
}
// The scene is being edited in place: the frames in flight end as above -- they show the scene as it was -- but a frame found
// skipped stays pending for the next splat_sync, as for every call that quiesces on its way to something else.
int end_frames_for_edit(splat_ctx* c) {
    bump_epoch(c);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = finish_quiet(c);
    if (rc != SPLAT_OK) return rc;
    return sync_all(c);
}
// Other values under every tile: what the region layouts, the sort launch sizes, the walks of the old ones (near selection,
// start hints) and the frame policy remember says nothing any more.
void scene_edited(splat_ctx* c) {
    for (Slot& sl : c->slots) sl.layout_valid = false;
    c->sort_hint = false;
    if (c->need_hint && c->m_alloc) (void)fill_now(c->need_hint, 0, hint_table(c).bytes());
    reset_policy(c);
}
// Another scene altogether: the context's per-scene state starts over, the per-tile arrays and key buffers exist.
void scene_installed(splat_ctx* c, uint64_t n) {
    c->n = n;
    c->region_mult = 0;
    c->bucket_failed = false;              // key storage is sized at the first frame (prepare_binning)
    scene_edited(c);
    // The per-tile arrays (a few hundred KB per frame slot at 4K) exist before the first frame as well: fifty small allocations
    // and six synchronous fills were a third of its call.  A larger target than 3840 x 2160 makes them again, as always.
    if (c->m_alloc == 0 && ensure_bins(c, 240u * 135u) != SPLAT_OK) (void)hipGetLastError();
    // The key buffers of one-pass binning depend on the scene's size only: made here, not inside the first frame's call (1.5 GB
    // of hipMalloc on C3).  A failure is left to the first frame, which retries smaller sizes (prepare_binning).
    if (c->use_buckets && !c->cfg.pair_capacity && !c->bucket_failed) {
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(c->cap, region_capacity_for(c, default_region_multiplier(c))), KEY_ENTRIES_MAX);
        const uint64_t want2 = std::min<uint64_t>(std::max<uint64_t>(c->cap2, default_keys2_capacity(c)), KEY_ENTRIES_MAX);
        if ((want + want2) * 8ull * (uint64_t)slots_in_use(c) <= c->bucket_bytes && ensure_keys(c, want, want2) != SPLAT_OK) (void)hipGetLastError();
    }
}
// A view's tile lists for a scene query, outside any frame: what splat_tile_row_loads does (K1's counting flavour and the scan
// into slot 0, the slab ignored), then -- the pair count and the list-length classes read back -- the emit into key buffers
// sized exactly and the sort launches with every list of two keys or more in them (fused_sort_max = 0: the short ones too;
// the grids are the scan's own prefixes of the longest-first order).  No block culling: a query wants every record K1 makes.
int bin_view_for_query(splat_ctx* c, const splat_camera* cam, ViewLists* out) {
    *out = ViewLists{};
    int rc = finish_quiet(c);
    if (rc != SPLAT_OK) return rc;
    const int s0 = c->slab0, s1 = c->slab1;
    c->slab0 = 0; c->slab1 = -1;
    FrameConst fc; unsigned int nt = 0;
    rc = build_frame_const(c, cam, &fc, &nt);
    c->slab0 = s0; c->slab1 = s1;
    if (rc != SPLAT_OK) return rc;
    fc.bucket_cap = 0; fc.cull_blocks = 0;
    out->fc = fc; out->n_tiles = nt;
    if (c->n == 0 || nt == 0) return SPLAT_OK;
    rc = ensure_bins(c, nt);
    if (rc != SPLAT_OK) return rc;
    Slot& s = c->slots[0];
    rc = ensure_two_pass_buffers(c, s);
    if (rc != SPLAT_OK) return rc;
    bump_epoch(c);              // (the pass below writes the slot's records, tile table and counters)
    HIP_TRY(c, hipMemsetAsync(s.counts, 0, sizeof(unsigned int) * ((size_t)nt + 1), c->stream));   // (one-pass frames leave cursors there)
    s.layout_valid = false; s.flip = 0;                                                          // ... and will find them gone
    HIP_TRY(c, hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream));
    BinArgs k1{};       // (the counting flavour: no bounds, no block words, no layout, no keys)
    k1.s = c->stream; k1.knobs = &c->knobs; k1.scene = {c->n, c->planes, c->orig, nullptr}; k1.fc = fc; k1.recs = s.recs; k1.depth = s.depth;
    k1.rect = s.rect; k1.vislist = s.vislist; k1.bin.cursors = s.counts; k1.status = s.d_status;
    launch_preprocess(k1);
    const TileLists lists = {s.offsets, s.order, s.lens, s.cursor, nullptr, nullptr};
    ScanArgs scan{};
    scan.s = c->stream; scan.knobs = &c->knobs; scan.m = nt; scan.bin = k1.bin; scan.lists = lists;
    scan.keys.cap = ~0ull; scan.grids = {nt, nt, nt}; scan.status = s.d_status;
    launch_scan(scan);
    HIP_TRY(c, hipGetLastError());
    FrameStatus st{};
    HIP_TRY(c, hipMemcpyAsync(&st, s.d_status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (st.overflow != 0 || st.n_pairs >= KEY_ENTRIES_MAX) {
        (void)hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream);
        return fail(c, SPLAT_ERR_CAPACITY, "the view has more (Gaussian, tile) pairs than a key buffer can index");
    }
    if (st.n_pairs != 0) {
        hipError_t e = dmalloc(c, &out->keys, sizeof(unsigned long long) * st.n_pairs);
        // (the second buffer mirrors the first, list for list: the run merges and global radix passes of lists beyond 16384 keys)
        if (e == hipSuccess && st.max_tile_len > 16384u) e = dmalloc(c, &out->keys2, sizeof(unsigned long long) * st.n_pairs);
        if (e != hipSuccess) {
            dfree(out->keys); dfree(out->keys2);
            (void)hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream);
            return fail(c, SPLAT_ERR_HIP, std::string("hipMalloc(query key buffers): ") + hipGetErrorString(e));
        }
        EmitArgs emit{};
        emit.s = c->stream; emit.scene = scene_of(c); emit.fc = fc; emit.depth = s.depth; emit.rect = s.rect; emit.vislist = s.vislist;
        emit.cursor = s.cursor; emit.keys = out->keys; emit.status = s.d_status;
        launch_emit(emit);
        SortArgs sort{};
        sort.s = c->stream; sort.knobs = &c->knobs; sort.n_tiles = nt; sort.grids = {st.n_ge8192, st.n_ge2048, st.n_ge16384};
        sort.lists = lists; sort.keys.keys = out->keys; sort.keys.keys2 = out->keys2; sort.status = s.d_status; sort.orig = c->orig;
        sort.fused_sort_max = 0u;
        launch_sort(sort);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream);     // frames expect a zeroed status
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        dfree(out->keys); dfree(out->keys2);
        return fail(c, SPLAT_ERR_HIP, std::string("the query's binning: ") + hipGetErrorString(e));
    }
    out->recs = s.recs; out->rect = s.rect; out->offsets = s.offsets; out->lens = s.lens; out->n_pairs = st.n_pairs;
    return SPLAT_OK;
}
}  // namespace splat

extern "C" {

int splat_set_slab(splat_ctx* c, int32_t tile_row0, int32_t tile_row1) {
    if (!c) return SPLAT_ERR_INVALID;
    if (tile_row0 < 0 || (tile_row1 >= 0 && tile_row1 < tile_row0)) return fail(c, SPLAT_ERR_INVALID, "bad slab");
    if (tile_row0 == c->slab0 && tile_row1 == c->slab1) return SPLAT_OK;
    bump_epoch(c);
    // another slab: the slots' region layouts (sized from the lists of the OLD slab's tile rows -- a partition that keeps
    // the tile count would keep them otherwise) and the sort launch sizes describe other tiles.  The next frame counts its
    // pairs first (bootstrap) instead of being binned against them, overflowing and getting dropped on the device.
    int rc = SPLAT_OK;
    if (c->frame_idx != 0) {
        (void)hipSetDevice(c->cfg.device);
        rc = finish_quiet(c);
    }
    for (Slot& sl : c->slots) sl.layout_valid = false;
    c->sort_hint = false;
    c->hint_pairs = 0; c->hint_maxlen = 0;
    if (c->need_hint && c->m_alloc) (void)hipMemsetAsync(c->need_hint, 0, hint_table(c).bytes(), c->stream);
    c->slab0 = tile_row0; c->slab1 = tile_row1;
    reset_policy(c);
    return rc;
}

int splat_tile_row_loads(splat_ctx* c, const splat_camera* cam, uint64_t* row_pairs, int32_t n_rows) {
    if (!c) return SPLAT_ERR_INVALID;
    if (!row_pairs) return fail(c, SPLAT_ERR_INVALID, "row_pairs is NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = finish_quiet(c);
    if (rc != SPLAT_OK) return rc;
    const int s0 = c->slab0, s1 = c->slab1;
    c->slab0 = 0; c->slab1 = -1;
    FrameConst fc; unsigned int nt = 0;
    rc = build_frame_const(c, cam, &fc, &nt);
    c->slab0 = s0; c->slab1 = s1;
    if (rc != SPLAT_OK) return rc;
    if (n_rows != fc.n_tile_rows) return fail(c, SPLAT_ERR_INVALID, "n_rows must be ceil(h/16)");
    for (int r = 0; r < n_rows; ++r) row_pairs[r] = 0;
    if (c->n == 0 || nt == 0) return SPLAT_OK;
    rc = ensure_bins(c, nt);
    if (rc != SPLAT_OK) return rc;
    Slot& s = c->slots[0];
    rc = ensure_two_pass_buffers(c, s);
    if (rc != SPLAT_OK) return rc;
    bump_epoch(c);              // (the pass below writes the slot's records, tile table and counters)
    fc.bucket_cap = 0;          // count only
    HIP_TRY(c, hipMemsetAsync(s.counts, 0, sizeof(unsigned int) * ((size_t)nt + 1), c->stream));   // (one-pass frames leave cursors there)
    s.layout_valid = false; s.flip = 0;                                                          // ... and will find them gone
    HIP_TRY(c, hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream));
    BinArgs k1{};       // (the counting flavour: no layout, no keys)
    k1.s = c->stream; k1.knobs = &c->knobs; k1.scene = scene_of(c); k1.fc = fc; k1.recs = s.recs; k1.depth = s.depth; k1.rect = s.rect; k1.vislist = s.vislist;
    k1.bin.cursors = s.counts; k1.blockinfo = s.blockinfo; k1.status = s.d_status;
    launch_preprocess(k1);
    ScanArgs scan{};
    scan.s = c->stream; scan.knobs = &c->knobs; scan.m = nt; scan.bin = k1.bin; scan.lists = {s.offsets, s.order, s.lens, s.cursor, nullptr, nullptr};
    scan.keys.cap = ~0ull; scan.grids = {nt, nt, nt}; scan.status = s.d_status;
    launch_scan(scan);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned int> off((size_t)nt + 1);
    HIP_TRY(c, hipMemcpyAsync(off.data(), s.offsets, sizeof(unsigned int) * off.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream));     // frames expect a zeroed status
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_rows; ++r)
        row_pairs[r] = (uint64_t)off[(size_t)(r + 1) * fc.tiles_x] - (uint64_t)off[(size_t)r * fc.tiles_x];
    return SPLAT_OK;
}

}  // extern "C"

namespace {
// host_out != nullptr (splat_render_frame): the rendered rows also travel to host memory behind the compositor, on its stream,
// BEFORE the host waits -- one wait per frame; a frame the device skipped is redone and copied again
int render_device_impl(splat_ctx* c, const splat_camera* cam, void* d_argb, int32_t sync, splat_stats* stats, bool clear_first,
                       uint32_t* host_out = nullptr) {
    if (!c) return SPLAT_ERR_INVALID;
    if (!d_argb) return fail(c, SPLAT_ERR_INVALID, "d_argb is NULL");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = SPLAT_OK;
    if (c->n == 0 && !c->planes) {
        // an empty scene renders nothing (the reference's loop body never runs); a viewer-loop frame is still cleared
        unsigned int nt;
        rc = build_frame_const(c, cam, &c->fc, &nt);
        if (rc) return rc;
        if (c->pre_wait) { HIP_TRY(c, hipStreamWaitEvent(c->stream, c->pre_wait, 0)); c->pre_wait = nullptr; }
        c->last_lane = 0;
        if (clear_first && c->fc.row_px1 > c->fc.row_px0) {
            HIP_TRY(c, hipMemsetAsync((uint32_t*)d_argb + (size_t)c->fc.row_px0 * c->fc.W, 0,
                                      (size_t)(c->fc.row_px1 - c->fc.row_px0) * c->fc.W * 4, c->stream));
            if (sync || stats) HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (host_out) std::memset(host_out + (size_t)c->fc.row_px0 * c->fc.W, 0, (size_t)(c->fc.row_px1 - c->fc.row_px0) * c->fc.W * 4);
        }
        if (stats) { c->last = FrameStatus{}; c->last_ring = -1; fill_stats(c, stats); }
        return SPLAT_OK;
    }
    rc = build_frame_const(c, cam, &c->fc, &c->n_tiles);
    if (rc != SPLAT_OK) return rc;
    if (c->n_tiles == 0) { if (stats) { c->last = FrameStatus{}; c->last_ring = -1; fill_stats(c, stats); } return SPLAT_OK; }
    rc = ensure_bins(c, c->n_tiles);
    if (rc != SPLAT_OK) return rc;
    for (int attempt = 0; attempt < 4; ++attempt) {
        rc = prepare_binning(c, c->n_tiles, &c->fc);
        if (rc != SPLAT_OK) return rc;
        const bool timed = stats != nullptr || c->timing_every <= 1 || (c->frame_idx % (uint64_t)c->timing_every) == 0;
        c->clear_first = clear_first;
        rc = enqueue_frame(c, cam, (uint32_t*)d_argb, timed, stats != nullptr, !sync && !stats && c->comp2 != nullptr && c->overlap >= 2 && !c->streamed_call,
                           sync || stats != nullptr);
        c->clear_first = false;
        if (rc != SPLAT_OK) return rc;
        if (host_out && c->fc.row_px1 > c->fc.row_px0) {
            const size_t first = (size_t)c->fc.row_px0 * (size_t)c->fc.W, count = (size_t)(c->fc.row_px1 - c->fc.row_px0) * (size_t)c->fc.W;
            HIP_TRY(c, copy_to_host_image(host_out + first, (const uint32_t*)d_argb + first, count * 4u, frame_stream(c)));
        }
        if (!sync && !stats) return SPLAT_OK;
        bool skipped = false;
        rc = finish_frame(c, &skipped);
        {   // frames lost besides this one (older asynchronous frames) are reported by the next splat_sync
            const uint64_t pending = c->frames_dropped - c->frames_drop_reported;
            if (pending > (skipped ? 1u : 0u)) c->deferred_drop = true;
            c->frames_drop_reported = c->frames_dropped;
        }
        if (rc != SPLAT_ERR_CAPACITY) break;
        if (!skipped) {
            // THIS frame composited; what was lost is an older asynchronous frame.  Redoing the frame would
            // blend it onto the in/out image a second time: report the loss at the next splat_sync instead.
            c->deferred_drop = true;
            rc = SPLAT_OK;
            break;
        }
        // this frame was skipped on the device; its storage has been grown / its path switched: redo
        if (!(c->fc.bucket_cap || c->last.overflow == 3 || c->cap > c->last.n_pairs)) break;
    }
    if (rc != SPLAT_OK) return rc;
    if (stats) fill_stats(c, stats);
    return SPLAT_OK;
}
}  // namespace

extern "C" {

int splat_render_device(splat_ctx* c, const splat_camera* cam, void* d_argb, int32_t sync, splat_stats* stats) {
    return render_device_impl(c, cam, d_argb, sync, stats, false);
}
int splat_render_frame_device(splat_ctx* c, const splat_camera* cam, void* d_argb, int32_t sync, splat_stats* stats) {
    return render_device_impl(c, cam, d_argb, sync, stats, true);
}

int splat_render(splat_ctx* c, const splat_camera* cam, uint32_t* argb, splat_stats* stats) {
    if (!c) return SPLAT_ERR_INVALID;
    if (!argb || !cam) return fail(c, SPLAT_ERR_INVALID, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    FrameConst fc; unsigned int nt;
    int rc = build_frame_const(c, cam, &fc, &nt);
    if (rc != SPLAT_OK) return rc;
    size_t bytes = (size_t)fc.W * fc.H * 4;
    if (bytes > c->img_cap) {
        (void)finish_quiet(c);
        dfree(c->d_img); c->img_cap = 0;
        HIP_TRY(c, dmalloc(c, &c->d_img, bytes));
        c->img_cap = bytes;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_img, argb, bytes, hipMemcpyHostToDevice, c->stream));
    rc = splat_render_device(c, cam, c->d_img, 1, stats);
    if (rc != SPLAT_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(argb, c->d_img, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

// The viewer loop's frame, host-visible and synchronous: `color.clear(0); render_to_buffer(&mut color)` (src/main.rs:73-74)
// as ONE call that ships no zeros.  splat_render uploads the caller's image (8.3 MB of zeros at 1080p), blends, downloads;
// here the clear is fused into the compositor and the pixels cross PCIe once, device -> host:
//   * a page-locked `argb_out` (splat_host_alloc / splat_host_register) whose memory the device can address is written by the
//     COMPOSITOR ITSELF (zero copy: the image crosses PCIe while the frame is still being composited; SPLAT_OPT_HOST_ZERO_COPY),
//   * any other `argb_out` gets a copy behind the compositor on its stream (page-locked: DMA at the PCIe rate; pageable: the
//     driver's staged copy).
int splat_render_frame(splat_ctx* c, const splat_camera* cam, uint32_t* argb_out, splat_stats* stats) {
    if (!c) return SPLAT_ERR_INVALID;
    if (!argb_out || !cam) return fail(c, SPLAT_ERR_INVALID, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    FrameConst fc; unsigned int nt;
    int rc = build_frame_const(c, cam, &fc, &nt);
    if (rc != SPLAT_OK) return rc;
    const size_t bytes = (size_t)fc.W * fc.H * 4;
    if (c->host_zero_copy) {
        // is this image page-locked and mapped into the device's address space?  (pageable memory: the query fails)
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof at);
        void* dev = nullptr;
        if (hipPointerGetAttributes(&at, argb_out) == hipSuccess && at.type == hipMemoryTypeHost &&
            hipHostGetDevicePointer(&dev, argb_out, 0) == hipSuccess && dev != nullptr &&
            host_range_is_locked(argb_out, dev, bytes))      // (the WHOLE image, not its first byte: a store past a mapping is a GPU page fault)
            return render_device_impl(c, cam, dev, 1, stats, true);      // the sync at the end of the frame makes the stores visible
        (void)hipGetLastError();
    }
    if (bytes > c->img_cap) {
        (void)finish_quiet(c);
        dfree(c->d_img); c->img_cap = 0;
        HIP_TRY(c, dmalloc(c, &c->d_img, bytes));
        c->img_cap = bytes;
    }
    return render_device_impl(c, cam, c->d_img, 1, stats, true, argb_out);
}

int splat_render_stream(splat_ctx* c, const splat_camera* cam, uint32_t* argb_out) {
    if (!c) return SPLAT_ERR_INVALID;
    if (!argb_out || !cam) return fail(c, SPLAT_ERR_INVALID, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    FrameConst fc; unsigned int nt;
    int rc = build_frame_const(c, cam, &fc, &nt);
    if (rc != SPLAT_OK) return rc;
    const size_t bytes = (size_t)fc.W * fc.H * 4;
    HIP_TRY(c, ensure_copy_stream(c));
    if (bytes > c->s_cap) {
        rc = sync_all(c);
        if (rc != SPLAT_OK) return rc;
        for (int k = 0; k < splat_ctx::S_IMGS; ++k) {
            dfree(c->s_img[k]); c->s_used[k] = false;
            HIP_TRY(c, dmalloc(c, &c->s_img[k], bytes));
            HIP_TRY(c, fill_now(c->s_img[k], 0, bytes));      // a slab context renders its own rows only: the rest reads as zeros
        }
        c->s_cap = bytes;
    }
    const int k = (int)(c->s_idx++ % (uint64_t)splat_ctx::S_IMGS);
    // the image must not be cleared while its previous frame is still crossing PCIe: the compositor waits for that copy.
    // (Streamed frames stay on lane 0 whatever the frame overlap: lane 1's stream is the one their copies travel on.)
    c->pre_wait = c->s_used[k] ? c->s_copied[k] : nullptr;
    c->streamed_call = true;
    rc = splat_render_frame_device(c, cam, c->s_img[k], 0, nullptr);      // clear + render (the clear is fused into the compositor)
    c->streamed_call = false;
    if (c->pre_wait) {      // no frame was enqueued (an error, a target without tiles): nothing of this call may run ahead of the copy
        (void)hipStreamWaitEvent(c->stream, c->pre_wait, 0);
        c->pre_wait = nullptr; c->last_lane = 0;
    }
    if (rc != SPLAT_OK) return rc;
    c->s_ring[k] = c->last_ring; c->s_cam[k] = *cam;
    HIP_TRY(c, hipEventRecord(c->s_rendered[k], frame_stream(c)));
    HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->s_rendered[k], 0));
    HIP_TRY(c, hipMemcpyAsync(argb_out, c->s_img[k], bytes, hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(c, hipEventRecord(c->s_copied[k], c->copy_stream));
    c->s_dst[k] = argb_out; c->s_used[k] = true;
    return SPLAT_OK;
}

int splat_stream_wait(splat_ctx* c, const uint32_t* argb_out) {
    if (!c) return SPLAT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // the most recent frame that went to this buffer (the other image may hold an older one)
    for (int j = 1; j <= splat_ctx::S_IMGS; ++j) {
        const int k = (int)((c->s_idx + (uint64_t)(splat_ctx::S_IMGS - j)) % (uint64_t)splat_ctx::S_IMGS);    // newest first
        if (c->s_used[k] && c->s_dst[k] == argb_out) {
            HIP_TRY(c, hipEventSynchronize(c->s_copied[k]));
            // The frame's status arrived before its pixels left.  If it was skipped on the device (it outgrew
            // its tile buckets / the sort launches sized from an earlier frame), grow the storage and render
            // it again, synchronously, into the same buffer: a viewer loop never sees the miss.
            const int r = c->s_ring[k];
            const bool skipped = r >= 0 && c->h_status[r].overflow != 0;
            if (!skipped) return SPLAT_OK;
            int rc = finish_quiet(c);                 // every frame in flight lands; storage grown
            if (rc != SPLAT_OK) return rc;
            {   // Streamed losses are redone by their own waits (this one below, the other images' by theirs: their status
                // words say so) and are therefore settled here; only a loss that belongs to NO streaming image -- a
                // plain asynchronous splat_render_device frame in flight beside the stream -- stays pending for the
                // next splat_sync.  (Without this the synchronous redo below found `dropped - reported >= 1` with its
                // own frame complete and left a spurious SPLAT_ERR_CAPACITY behind for the next splat_sync.)
                uint64_t streamed = 0;
                for (int q = 0; q < splat_ctx::S_IMGS; ++q)
                    if (c->s_used[q] && c->s_ring[q] >= 0 && c->h_status[c->s_ring[q]].overflow != 0) ++streamed;
                const uint64_t pending = c->frames_dropped - c->frames_drop_reported;
                c->deferred_drop = pending > streamed;
                c->frames_drop_reported = c->frames_dropped;
            }
            const size_t bytes = (size_t)c->s_cam[k].w * (size_t)c->s_cam[k].h * 4;
            const bool other_pending = c->deferred_drop;
            rc = splat_render_frame_device(c, &c->s_cam[k], c->s_img[k], 1, nullptr);
            if (rc != SPLAT_OK) return rc;
            c->deferred_drop = other_pending;          // (the redo's own bookkeeping saw only settled streamed losses)
            c->s_ring[k] = c->last_ring;
            HIP_TRY(c, hipMemcpyAsync(const_cast<uint32_t*>(argb_out), c->s_img[k], bytes, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return SPLAT_OK;
        }
    }
    return fail(c, SPLAT_ERR_INVALID, "no streamed frame is bound to this buffer");
}

void* splat_device_alloc(splat_ctx* c, uint64_t bytes) {
    if (!c) return nullptr;
    void* p = nullptr;
    hipError_t e = hipSetDevice(c->cfg.device);
    if (e == hipSuccess) e = dmalloc(c, &p, (size_t)std::max<uint64_t>(bytes, 1));
    if (e != hipSuccess) { c->err = std::string("splat_device_alloc: ") + hipGetErrorString(e); return nullptr; }
    return p;
}
void splat_device_free(splat_ctx* c, void* p) {
    if (!c || !p) return;
    (void)hipSetDevice(c->cfg.device);
    (void)sync_all(c);                      // frames in flight may still be writing the image
    ledger_del(p);
    (void)hipFree(p);
}
int splat_device_upload(splat_ctx* c, void* d_dst, const void* h_src, uint64_t bytes) {
    if (!c) return SPLAT_ERR_INVALID;
    if (bytes && (!d_dst || !h_src)) return fail(c, SPLAT_ERR_INVALID, "NULL pointer");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, join_lanes(c));
    HIP_TRY(c, hipMemcpyAsync(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}
int splat_device_download(splat_ctx* c, void* h_dst, const void* d_src, uint64_t bytes) {
    if (!c) return SPLAT_ERR_INVALID;
    if (bytes && (!h_dst || !d_src)) return fail(c, SPLAT_ERR_INVALID, "NULL pointer");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, join_lanes(c));
    HIP_TRY(c, hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPLAT_OK;
}

void* splat_host_alloc(uint64_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, (size_t)bytes) != hipSuccess) return nullptr;
    host_range_add(p, (size_t)bytes);
    return p;
}
void splat_host_free(void* p) { if (p) { host_range_del(p); (void)hipHostFree(p); } }
int splat_host_register(void* p, uint64_t bytes) {
    if (!p || !bytes) return SPLAT_ERR_INVALID;
    if (hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault) != hipSuccess) return SPLAT_ERR_HIP;
    host_range_add(p, (size_t)bytes);
    return SPLAT_OK;
}
int splat_host_unregister(void* p) {
    if (!p) return SPLAT_ERR_INVALID;
    host_range_del(p);
    return hipHostUnregister(p) == hipSuccess ? SPLAT_OK : SPLAT_ERR_HIP;
}

int splat_sync(splat_ctx* c) {
    if (!c) return SPLAT_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return finish_and_report(c);
}

uint64_t splat_frames_dropped(const splat_ctx* c) { return c ? c->frames_dropped : 0; }

int splat_frames_retained(splat_ctx* c, uint64_t* n) {
    if (!c || !n) return SPLAT_ERR_INVALID;
    *n = c->frames_retained;
    return SPLAT_OK;
}

uint64_t splat_device_bytes(const splat_ctx* c, uint64_t* peak) {
    if (!c) return 0;
    if (peak) *peak = c->dev_bytes_peak;
    return c->dev_bytes;
}

int splat_get_timing(splat_ctx* c, double ms_out[6], uint64_t* frames, int32_t reset) {
    if (!c) return SPLAT_ERR_INVALID;
    int rc = splat_sync(c);
    if (rc != SPLAT_OK) return rc;
    if (ms_out) for (int k = 0; k < N_TIMES; ++k) ms_out[k] = c->acc_ms[k];
    if (frames) *frames = c->acc_frames;
    if (reset) { for (auto& v : c->acc_ms) v = 0; c->acc_frames = 0; }
    return SPLAT_OK;
}

int splat_get_records(splat_ctx* c, splat_record* out, uint64_t n) {
    if (!c || !out) return SPLAT_ERR_INVALID;
    if (n != c->n) return fail(c, SPLAT_ERR_INVALID, "record count mismatch");
    if (n == 0) return SPLAT_OK;
    int rc = splat_sync(c);
    if (rc != SPLAT_OK) return rc;
    if (c->last_slot < 0) return fail(c, SPLAT_ERR_INVALID, "no frame rendered yet");
    rc = ensure_two_pass_buffers(c, c->slots[c->last_slot]);
    if (rc != SPLAT_OK) return rc;
    const Slot& s = c->slots[c->last_slot];
    // The 48-byte records are the ones the frame itself was composited from (written by whichever flavour of K1
    // rendered it -- preprocess_kernel<true> on the default one-pass path); they are read FIRST.
    std::vector<Rec> r(n); std::vector<float> d(n); std::vector<ushort4> q(n);
    HIP_TRY(c, hipMemcpy(r.data(), s.recs, sizeof(Rec) * n, hipMemcpyDeviceToHost));
    {
        // Depth and pixel rectangle exist only in registers on the one-pass path, and block culling skips whole
        // blocks (whose records above are then stale, for Gaussians that reach nothing): recompute those two with
        // the counting flavour of K1, culling off (same code, same values), then clear its counts again.
        bump_epoch(c);          // (the pass below writes the slot's records and counters)
        FrameConst fc = c->fc;
        fc.bucket_cap = 0; fc.cull_blocks = 0;
        Slot& sl = c->slots[c->last_slot];
        HIP_TRY(c, hipMemsetAsync(sl.counts, 0, sizeof(unsigned int) * ((size_t)c->n_tiles + 1), c->stream));   // (cursors of a one-pass frame)
        sl.layout_valid = false; sl.flip = 0;
        HIP_TRY(c, hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream));
        BinArgs k1{};       // (no bounds, no block words, no layout, no keys)
        k1.s = c->stream; k1.knobs = &c->knobs; k1.scene = {c->n, c->planes, c->orig, nullptr}; k1.fc = fc; k1.recs = s.recs; k1.depth = s.depth; k1.rect = s.rect;
        k1.vislist = s.vislist; k1.bin.cursors = s.counts; k1.status = s.d_status;
        launch_preprocess(k1);
        HIP_TRY(c, hipMemsetAsync(s.counts, 0, sizeof(unsigned int) * ((size_t)c->n_tiles + 1), c->stream));
        HIP_TRY(c, hipMemsetAsync(s.d_status, 0, sizeof(FrameStatus), c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    HIP_TRY(c, hipMemcpy(d.data(), s.depth, sizeof(float) * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(q.data(), s.rect, sizeof(ushort4) * n, hipMemcpyDeviceToHost));
    rc = ensure_h_orig(c);
    if (rc != SPLAT_OK) return rc;
    for (uint64_t j = 0; j < n; ++j) {          // everything lives in slot order; the caller gets original order
        const uint64_t i = c->h_orig[j];
        splat_record& o = out[i];
        // K1 stores a record only for a Gaussian that reaches the slab's rows (in_slab); the slot's word for any other is
        // whatever an earlier frame or the allocation left there: such a record reads as zeros, in every slot alike
        const bool on_target = q[j].x <= q[j].y && q[j].z <= q[j].w;
        if (!(on_target && std::max((int)q[j].z, c->fc.row_px0) <= std::min((int)q[j].w, c->fc.row_px1 - 1))) r[j] = Rec{};
        o.cx = r[j].a.x; o.cy = r[j].a.y; o.hx = r[j].a.z; o.hy = r[j].a.w;
        o.conic_a = r[j].b.x; o.conic_b = c->fc.y_up ? r[j].b.y : -r[j].b.y; o.conic_c = r[j].b.z; o.opacity = r[j].b.w;
        o.r = r[j].c.x; o.g = r[j].c.y; o.b = r[j].c.z; o.depth = d[j];
        o.px0 = q[j].x; o.px1 = q[j].y; o.py0 = q[j].z; o.py1 = q[j].w;
    }
    return SPLAT_OK;
}

#if SPLAT_K1X == 30 || SPLAT_K1X == 31
int splat_debug_k1_stamps(splat_ctx* c, unsigned long long* out, unsigned long long n_words) {
    if (!c || c->last_slot < 0) return SPLAT_ERR_INVALID;
    (void)sync_all(c);
    return hipMemcpy(out, c->slots[c->last_slot].depth, n_words * 8, hipMemcpyDeviceToHost) == hipSuccess ? SPLAT_OK : SPLAT_ERR_HIP;
}
int splat_debug_k1_hwid(splat_ctx* c, unsigned long long* out, unsigned long long n_words) {
    if (!c || c->last_slot < 0) return SPLAT_ERR_INVALID;
    (void)sync_all(c);
    return hipMemcpy(out, c->slots[c->last_slot].rect, n_words * 8, hipMemcpyDeviceToHost) == hipSuccess ? SPLAT_OK : SPLAT_ERR_HIP;
}
#endif

// (debug, not part of the ABI)  The near selection's per-tile state of the most recent frame: lens[m], near_m[m], need_hint[4 m].
int splat_debug_near_state(splat_ctx* c, unsigned int* lens, unsigned int* near_m, unsigned int* need_hint, unsigned int m) {
    if (!c || c->last_slot < 0 || m != c->n_tiles) return SPLAT_ERR_INVALID;
    (void)sync_all(c);
    const Slot& s = c->slots[c->last_slot];
    bool ok = hipMemcpy(lens, s.lens, sizeof(unsigned int) * m, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(near_m, s.near_m, sizeof(unsigned int) * m, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(need_hint, hint_table(c).needs(), sizeof(unsigned int) * HintTable::NEED_PLANES * m, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? SPLAT_OK : SPLAT_ERR_HIP;
}

// (debug, not part of the ABI)  Waves of the last harvested statistics frame whose start-refinement probe did not close its
// bracket and walked again from the known-good start (FrameStatus::n_probe_fail; not among splat_stats::n_fallback).
int splat_debug_probe_failures(splat_ctx* c, uint64_t* n) {
    if (!c || !n || c->last_slot < 0) return SPLAT_ERR_INVALID;
    *n = c->last.n_probe_fail;
    return SPLAT_OK;
}

int64_t splat_binning_mode(splat_ctx* c) {
    if (!c || c->last_slot < 0) return -1;
    return (int64_t)c->fc.bucket_cap;
}

int splat_get_tile_lists(splat_ctx* c, uint32_t* tile_offsets, uint64_t n_offsets, uint32_t* order, uint64_t n_order) {
    if (!c) return SPLAT_ERR_INVALID;
    int rc = splat_sync(c);
    if (rc != SPLAT_OK) return rc;
    if (c->last_slot < 0) return fail(c, SPLAT_ERR_INVALID, "no frame rendered yet");
    if (!c->last_lists_in_memory)
        return fail(c, SPLAT_ERR_INVALID, "the last frame kept its sorted short lists on chip: render it with a stats pointer to read the lists");
    const Slot& s = c->slots[c->last_slot];
    if (n_offsets != (uint64_t)c->n_tiles + 1 || n_order != c->last.n_pairs)
        return fail(c, SPLAT_ERR_INVALID, "tile list size mismatch");
    if (c->last_near && c->last.overflow == 0) {
        // the frame's compositor selected the nearest keys of every list of more than 2048 keys and left the list itself
        // as K1 had written it: put those lists in order now (the sort launches, every tile in their grids)
        bump_epoch(c);          // (the selections a retained frame would read are scatter space of these sorts)
        SortArgs sort{};
        sort.s = c->stream; sort.knobs = &c->knobs; sort.n_tiles = c->n_tiles; sort.grids = {c->n_tiles, c->n_tiles, c->n_tiles};
        sort.lists = {s.offsets, s.order, s.lens, s.cursor, c->fc.bucket_cap ? s.off2 : nullptr, s.near_m};
        sort.keys.keys = s.keys; sort.keys.keys2 = s.keys2; sort.status = s.d_status; sort.orig = c->orig; sort.fused_sort_max = 2048u;
        launch_sort(sort);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->last_near = false;
    }
    const size_t m = c->n_tiles;
    std::vector<unsigned int> beg(m + 1), len(m + 1);
    HIP_TRY(c, hipMemcpy(beg.data(), s.offsets, sizeof(unsigned int) * (m + 1), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(len.data(), s.lens, sizeof(unsigned int) * m, hipMemcpyDeviceToHost));
    uint64_t run = 0;
    for (size_t t = 0; t < m; ++t) { tile_offsets[t] = (uint32_t)run; run += len[t]; }
    tile_offsets[m] = (uint32_t)run;
    if (run != n_order) return fail(c, SPLAT_ERR_INVALID, "tile list size mismatch");
    if (n_order) {
        std::vector<unsigned long long> k(n_order);
        if (!c->fc.bucket_cap) {
            HIP_TRY(c, hipMemcpy(k.data(), s.keys, sizeof(unsigned long long) * n_order, hipMemcpyDeviceToHost));
        } else {                    // lists live in fixed-stride buckets: gather them
            for (size_t t = 0; t < m; ++t)
                if (len[t])
                    HIP_TRY(c, hipMemcpy(k.data() + tile_offsets[t], s.keys + beg[t], sizeof(unsigned long long) * len[t],
                                         hipMemcpyDeviceToHost));
        }
        rc = ensure_h_orig(c);
        if (rc != SPLAT_OK) return rc;
        for (uint64_t i = 0; i < n_order; ++i) order[i] = c->h_orig[(uint32_t)k[i]];      // keys carry slots
    }
    return SPLAT_OK;
}

}  // extern "C"
