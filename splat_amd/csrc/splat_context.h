// splat_context.h -- private to the library's host translation units (splat_api.hip: the frame scheduler, the render entry
// points, the options; splat_scene.hip: everything that puts values into the resident scene): the context, how both check a
// HIP call and own device memory, and the seam between the two.  splat_multi.hip stays outside: it sees a context through
// the accessor hooks of splat_internal.h only.
#ifndef SPLAT_CONTEXT_H
#define SPLAT_CONTEXT_H
#include <string>
#include <vector>

#include "splat_internal.h"
#include "../../include/splat_policy.h"
#include "../../include/splat_retain.h"

#define HIP_TRY(ctx, expr)                                                                             \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
            return SPLAT_ERR_HIP;                                                                      \
        }                                                                                              \
    } while (0)

namespace splat {
constexpr int N_EV = 9;        // e0..e2 on the bin stream (start, K1, scan), e8, e3, e4 on the sort stream (start, K2, K3), e5..e7 on the caller's (K4 start, K4 end, status)
constexpr int N_TIMES = 6;     // preprocess, scan, emit, sort, composite, status read-back
constexpr int EV_RING = 32;
static_assert(EV_RING == SPLAT_POLICY_RING, "the frame policy sees the whole status ring");
constexpr int N_SLOTS = 4;

struct EvSet {
    hipEvent_t e[N_EV];
    bool used = false;
    bool timed = false;        // the per-kernel events e0..e6, e8 were recorded for this frame
    bool retained = false;     // ... of which a retained frame (splat_retain.h) records e5, e6 only: the others are an older frame's
};

struct Slot {                  // everything one frame writes before the image
    Rec* recs = nullptr;
    float* depth = nullptr;
    ushort4* rect = nullptr;
    unsigned int* vislist = nullptr;
    unsigned int* counts = nullptr;        // per tile: pair count (two-pass binning, zero between frames) / cursor of the tile's region (one-pass)
    unsigned int* counts_b = nullptr;      // one-pass binning: cursors and regions exist twice per slot -- the layout of the slot's NEXT frame
    unsigned int* lay_a = nullptr;         // is written (layout_kernel of an earlier frame on the same stream) while nothing reads that copy
    unsigned int* lay_b = nullptr;
    int flip = 0;                          // which copy the slot's next frame uses (0: counts / lay_a, 1: counts_b / lay_b)
    bool layout_valid = false;             // ... and whether it holds regions for the current scene / target / slab
    unsigned int* offsets = nullptr;
    unsigned int* cursor = nullptr;
    unsigned int* order = nullptr;
    unsigned int* lens = nullptr;           // list length per tile (the list starts at offsets[tile])
    // Binning again on the device (overflow redo): counters, regions and cursors of a frame whose lists outgrew the regions
    // it was given -- its second binning pass writes here, not into the copies the pipeline hands on
    unsigned int* redo_layout = nullptr;
    unsigned int* redo_cursors = nullptr;
    uint64_t layout_cam[2] = {0, 0};        // per copy of the layout: a hash of the camera whose lists sized it
    unsigned int* near_m = nullptr;         // near selection: per tile, how many of its list's nearest keys launch_select put in order
    unsigned long long* keys = nullptr;
    unsigned long long* keys2 = nullptr;   // the second key buffer: sorted near selections, scatter space of the long lists' sorts and merges
    unsigned int* off2 = nullptr;          // one-pass binning: per tile, where its room in keys2 starts (handed out by the frame's scan to the
                                           // lists of more than 2048 keys; two-pass binning mirrors the first buffer instead)
    unsigned int* blockinfo = nullptr;     // per K1 block: the info word this slot's last K1 wrote (see launch_preprocess);
                                           // per slot, because the K1s of consecutive frames run concurrently
    uint4* large_list = nullptr;           // one-pass binning: the frame's large splats (key, tile rectangle), n entries -- K1 lists them,
    unsigned int* large_count = nullptr;   // bin_large_kernel bins them tile by tile; the counter is zero between frames (scan / layout reset it)
    FrameStatus* d_status = nullptr;
    hipEvent_t ev_binned = nullptr;        // bin stream -> sort stream: buckets and lengths are final
    hipEvent_t ev_ready = nullptr;         // sort stream -> caller's stream: lists are sorted
    int free_ring = -1;                    // compositor's stream -> bin stream: the slot is free when the frame that used it last has
                                           // ended -- that frame's ring event (an event of the slot's own would be a second barrier
                                           // packet behind every compositor: ~3 us of queue drain per frame)
    bool used = false;
};

// (none of what follows is the library's ABI: not exported, called directly)
#pragma GCC visibility push(hidden)
// the context's error string (the creating thread's without a context: splat_last_error(NULL)); returns `code`
int fail(splat_ctx* ctx, int code, const std::string& msg);

// Device allocations of a context go through these two, so that splat_device_bytes() can say what it holds (sizes are
// kept in a side table: hipFree does not tell).
void ledger_add(splat_ctx* c, void* p, size_t bytes);
void ledger_del(void* p);
template <typename T>
hipError_t dmalloc(splat_ctx* c, T** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) ledger_add(c, (void*)*p, bytes);
    return e;
}
template <typename T>
void dfree(T*& p) {
    if (p) { ledger_del((void*)p); (void)hipFree(p); p = nullptr; }
}

// hipMemset on device memory is ENQUEUED (on the legacy default stream) and may return before the fill has run -- and the
// context's streams are non-blocking: nothing on them waits for that stream.  A fill that the next launches depend on is
// waited for here.  (Found with eight processes on one GPU, where the default stream's fill arrives late: the first
// splat_tile_row_loads of two ranks in eight counted into counters that were zeroed afterwards -- tools/row_loads_stress.py.)
inline hipError_t fill_now(void* p, int value, size_t bytes) {
    hipError_t e = hipMemset(p, value, bytes);
    return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
}

// ---- The seam between the scene (splat_scene.hip) and the frame scheduler (splat_api.hip).  The scheduler keeps what it
// holds per scene -- region layouts, sort hints, the hint table, the policy's memory, key buffers -- to itself; the scene
// file tells it when frames must end and what became of the scene, and knows none of those by name.
int end_frames_for_upload(splat_ctx* c);     // the scene is being replaced: its frames end, nothing of them is left to redo or report
int end_frames_for_edit(splat_ctx* c);       // the scene is being edited: its frames end; one found skipped stays pending for splat_sync
void scene_edited(splat_ctx* c);             // other values under every tile: what the scheduler learnt from the old ones goes
void scene_installed(splat_ctx* c, uint64_t n);   // another scene of n Gaussians: scene_edited, and the per-tile arrays and key buffers exist
// A scene query that needs a view's tile lists (splat_visibility_device): the view binned like a two-pass frame over the whole
// target -- the frames in flight ended first, a slab ignored -- into the first frame slot's records and tile tables, every list
// in blend order in key buffers of the call's own: keys (and keys2, made only where a list needs it) are the CALLER's to
// dfree; nullptr with n_pairs == 0.  Everything is enqueued on the context's stream; the slot's counters and status are left
// zeroed, as frames expect them.
struct ViewLists {
    FrameConst fc; unsigned int n_tiles;
    const Rec* recs; const ushort4* rect; const unsigned int *offsets, *lens;
    unsigned long long *keys, *keys2; uint64_t n_pairs;
};
int bin_view_for_query(splat_ctx* c, const splat_camera* cam, ViewLists* out);
// ... and what the scheduler asks of the scene
void free_scene(splat_ctx* c);               // the scene's buffers and the frame slots' per-Gaussian ones go; n = 0
int ensure_h_orig(splat_ctx* c);             // c->h_orig holds the scene's order (the debug getters translate slots with it)
#pragma GCC visibility pop
}  // namespace splat

struct splat_ctx {
    splat_config cfg{};
    hipStream_t stream = nullptr;          // compositor + image: the caller-visible stream
    bool own_stream = false;
    hipStream_t bin_stream = nullptr;      // K1 + scan of a later frame
    hipStream_t sort_stream = nullptr;     // K2 + K3 (depth 2: the bin stream itself)
    // scene
    uint64_t n = 0;
    float4* planes = nullptr;
    unsigned int* orig = nullptr;          // slot -> original Gaussian index (Morton order of position)
    splat::BlockBounds* bounds = nullptr;  // per K1 block of 256 slots (block culling)
    bool cull_blocks = true;               // SPLAT_CULL=0 disables
    std::vector<unsigned int> h_orig;      // host copy of orig (ensure_h_orig: a device upload leaves it empty until a debug getter asks)
    // edits, transforms and reads by index (splat_*_gaussians_device): ONE allocation, made by the first such call on a scene and
    // freed with it -- inv[i] = the slot of Gaussian i (n words), the index check's counter, one dirty byte per K1 block
    unsigned int* inv = nullptr;
    unsigned int* upd_bad = nullptr;       // (inside inv's allocation)
    unsigned char* upd_dirty = nullptr;    // (likewise)
    float ply_ms[3] = {0.0f, 0.0f, 0.0f};  // device time of decode, sum, subtract inside the most recent PLY decode
    float upload_sort_ms = 0.0f;           // device time of the sort inside the most recent splat_upload_scene_device
    // per-frame buffers
    splat::Slot slots[splat::N_SLOTS];
    unsigned int m_alloc = 0;
    uint64_t cap = 0;                      // entries in each used slot's keys buffer
    uint64_t cap2 = 0;                     // entries in each used slot's second key buffer (0: none).  Two-pass binning: a mirror of the first
                                           // (cap2 == cap); one-pass: room for the lists of more than 2048 keys only (default_keys2_capacity)
    uint64_t keys2_want = 0;               // a harvested frame's long lists outgrew the second key buffer: grow to this
    // one-pass binning (per-tile regions of the key buffer, sized from earlier frames' lists): on unless SPLAT_BUCKETS=0, the
    // caller fixed pair_capacity, or the key buffers would not fit bucket_bytes
    bool use_buckets = true;
    bool bucket_failed = false;            // sticky until the scene changes
    uint64_t bucket_bytes = 128ull << 30;  // SPLAT_BUCKET_BYTES: all key buffers of all slots together (288 GB of HBM per GPU)
    uint64_t layout_want = 0;              // entries the regions of a harvested frame asked for and did not get (grow to this)
    unsigned int layout_m = 0;             // tile count the slots' layouts were built for
    bool last_one_pass = false;            // what the previous frame's binning was (the cursors must be zero for two-pass counting)
    unsigned int* zero_layout = nullptr;   // m_alloc zeros: the empty layout of the bootstrap (every key dropped, every pair counted)
    uint64_t dev_bytes = 0, dev_bytes_peak = 0;   // device memory held by this context
    splat::LaunchKnobs knobs;              // experiment switches of the launch wrappers (this context's)
    float region_spare = 4.0f;             // SPLAT_REGION_SPARE: how far a tile's region may grow into the key buffer's spare room (1: not at all)
    uint64_t frame_idx = 0;
    uint64_t bin_idx = 0;                  // frames BINNED so far: slots and binning streams rotate with these (a retained frame bins nothing)
    // Retained lists (include/splat_retain.h; enqueue_frame): with the camera at rest one frame -- the WRITER -- leaves every
    // list it composited from in order in memory (the compositor's write-back), and the frames behind it composite from its
    // slot alone until the camera's bytes or the binning epoch change.
    int retain_lists = 1;                  // SPLAT_OPT_RETAIN_LISTS / SPLAT_RETAIN
    uint64_t bin_epoch = 0;                // bumped wherever something a frame's binning or ordering reads or produces changes (bump_epoch)
    splat_retain_state ret{};
    uint64_t frames_retained = 0;
    struct RetainSet {                     // the writer: its slot and ring entry, how its long lists were ordered, its status as the scan left it
        int slot = -1, ring = -1;
        unsigned int near_cap = 0;
        splat::FrameStatus status{};
        unsigned int frames = 0;           // frames composited from the set so far (SPLAT_DBG_STAGE_CACHE=2 counts them)
    } ret_set;
    // The staging verdicts the set's frames keep for each other (CompArgs::stage_nv / stage_mask): per tile 4 counts and
    // 4 x 32 masks, m_alloc tiles, made when the first writer is launched, the counts cleared in front of every writer
    // ... and, behind the counts in the same allocation (one clear per writer), the starts the set has proven: one word per
    // (tile, wave) again (CompArgs::proven_start)
    unsigned int* stage_nv = nullptr;
    unsigned long long* stage_mask = nullptr;
    unsigned int* proven_start() const { return stage_nv ? stage_nv + (size_t)m_alloc * 4u : nullptr; }
    int last_slot = -1;                    // buffer slot of the most recent frame (debug getters)
    bool last_lists_in_memory = false;     // ... and whether its compositor wrote the lists it sorted back to the buckets
    splat::FrameStatus* h_status = nullptr;  // pinned, one per event-ring entry
    // Every frame in flight has a device status of its own (one per event-ring entry).  The scan kernel -- where a
    // frame's pair count, longest list and every overflow verdict are decided -- initialises it and writes the same
    // words straight into the pinned host copy, so an asynchronous frame needs no read-back and no reset on any
    // stream: the caller's stream carries nothing but the compositors back to back (a copy and two fills used to sit
    // between them, ~30 us per frame; a side stream for them shares a hardware queue with a binning stream and
    // serialises the frames).  Frames rendered with statistics still copy the final status (late counters).
    splat::FrameStatus* d_status_ring = nullptr;
    bool clear_first = false;              // the frame being enqueued starts from a cleared image (fused into the compositor)
    // host-image path
    uint32_t* d_img = nullptr;
    size_t img_cap = 0;
    // streaming path (splat_render_stream): two device images, a copy stream, per-image events
    static constexpr int S_IMGS = 4;       // streamed frames in flight (device images): the pipeline wants three (two chains + a compositor)
    uint32_t* s_img[S_IMGS] = {};
    size_t s_cap = 0;
    hipStream_t copy_stream = nullptr;
    hipEvent_t s_rendered[S_IMGS] = {}, s_copied[S_IMGS] = {};
    const uint32_t* s_dst[S_IMGS] = {};
    bool s_used[S_IMGS] = {};
    uint64_t s_idx = 0;
    int s_ring[S_IMGS] = {-1, -1, -1, -1}; // event-ring entry of the frame each streaming image holds
    splat_camera s_cam[S_IMGS] = {};       // ... and its camera (a frame skipped on the device is redone by splat_stream_wait)
    // slab
    int slab0 = 0, slab1 = -1;
    // timing
    splat::EvSet ring[splat::EV_RING];
    int ring_next = 0;
    int last_ring = -1;
    double acc_ms[splat::N_TIMES] = {0, 0, 0, 0, 0, 0};
    uint64_t acc_frames = 0;
    // last frame
    splat::FrameConst fc{};
    unsigned int n_tiles = 0;
    uint64_t overflow_want = 0;            // a harvested frame overflowed the pair buffer: grow to this
    bool bucket_overflow = false;          // a harvested frame overflowed a tile bucket: leave one-pass binning
    // sort launch sizes: the long-list sort launches cover a prefix of the longest-first tile order,
    // sized from the most recent harvested frame (+25 % + slack); the device validates, a miss redoes the frame
    bool sort_hint = false, sort_grid_miss = false;
    unsigned int hint_ge8192 = 0, hint_ge2048 = 0, hint_ge16384 = 0;
    // which flavour of the exact walk the compositor runs (the pixels are the same): 0 = one record per step, 1 = two
    // records per step with packed math (fewer issue slots: for frames whose compositor is bound by its longest
    // list's single wave, not by throughput), -1 = by the last harvested frame's pairs per key of the longest list
    int pair_mode = -1;                    // SPLAT_PAIR_BLEND
    uint64_t hint_pairs = 0; unsigned int hint_maxlen = 0; unsigned int hint_large = 0, hint_window = 0;
    unsigned int grid_big = 0, grid_mid = 0, grid_long = 0;      // what the frame being enqueued uses
    splat::FrameStatus last{};
    // frames skipped on the device (their storage outgrown: see finish_frame).  A synchronous call redoes its own
    // frame; a lost ASYNCHRONOUS frame is reported once, by the next splat_sync / splat_stream_wait
    uint64_t frames_dropped = 0, frames_drop_reported = 0;
    bool deferred_drop = false;
    bool tight_grids = false;              // SPLAT_DBG_TIGHT_GRIDS: sort launches sized with no margin (tests force a miss)
    uint2* d_iters = nullptr;              // per compositor wave: (scan, blend) iterations of a frame rendered with stats
    unsigned int iters_alloc = 0;
    bool iters_valid = false;
    // Who sorts the lists of more than 2048 keys: 0 = the sort launches (74 / 147 KB workgroups, starved beside a compositor
    // in flight, but the cheaper code), 1 = the tile's own compositor workgroup (no launches, no starvation, more
    // work), -1 = by the previous frame: the compositor when the AVERAGE list is longer than 2048 keys, i.e. when
    // the sort launches would carry most of the frame's keys, and the frame is throughput-bound (C5: +7 %; C3 -5 %, C2 -13 %
    // if forced).  SPLAT_SORT_IN_COMP.
    int sort_in_comp = -1;
    float fast_width = 2.0f;               // SPLAT_MODE_FAST: bracket width that counts as closed (SPLAT_FAST_WIDTH: 1 or 2)
    float early_eps = 1e-6f;               // SPLAT_EARLY_EPS overrides (0 disables the early-out)
    int early_min = 768;                   // SPLAT_EARLY_MIN
    int early_scan8 = 4;                   // SPLAT_EARLY_SCAN8
    int prio_len = 0x3fffffff;             // SPLAT_PRIO_LEN
    unsigned int fused_sort_max = 2048;    // SPLAT_FUSED_SORT: lists up to this length are sorted inside the compositor (0: off)
    // Near selection (SPLAT_NEAR_KEYS / SPLAT_OPT_NEAR_SELECT_KEYS; 0 = off): a list of more than 2048 keys is not sorted; its
    // tile's compositor workgroup selects the nearest <= near_cap keys by depth and sorts those -- the exact early-out never
    // looks farther on all but a few tiles, which then sort their whole list after all.  No sort launches in such frames.
    unsigned int near_cap = 2048;
    // Overflow redo (SPLAT_OVERFLOW_REDO / SPLAT_OPT_OVERFLOW_REDO, default on): a frame whose camera differs from the one its
    // tile regions were sized for carries a second binning (count pass, exact regions, K1, scan) behind its scan, as launches
    // that leave at once unless that scan found a tile beyond its region -- such a frame is binned again on the device
    // instead of being skipped, reported and rendered again by the caller.
    // 0 = off; 1 = ADAPTIVE (default): the redo launches ride on moving frames only while a list has outgrown its region within
    // the last 256 frames (a scene that never does -- most -- pays nothing; the first such frame after a quiet stretch is
    // skipped and reported as before, and arms the redo); 2 = on every moving frame.
    int overflow_redo = 1;
    // What the frame policy (include/splat_policy.h, splat_policy.cpp: a pure function, tested without a GPU) carries from frame
    // to frame: the previous camera and how long it has been the same, the count-first / overflow-redo runs left, how the frames
    // in the status ring were binned.  reset_policy() where the lists it speaks of stop existing (scene, target, slab, options).
    splat_policy_state pol{};
    // One-pass binning: splats of more tiles than this (and every splat wider or taller than K1's 32 x 32-tile window) go to the
    // frame's large list and are binned tile by tile behind K1 (bin_large_kernel).  SPLAT_LARGE_TILES: 0 = the window alone
    // decides, < 0 = no list at all (K1's blocks expand close-ups themselves, one atomic per pair: the round-5 path).
    int layout_motion = 1;               // SPLAT_LAYOUT_MOTION=0: regions always sized from each tile's own list (round 6)
    int large_list_min = 256;            // SPLAT_LARGE_LIST_MIN: large splats a recent frame must have had for frames to keep the list (splat_policy.h)
    int large_tiles = 128;               // (C2 / C3 / C5, bench pose and from inside: 96-128 best of 0..1024, profiles/r07_large_splats.txt)
    int count_first = 1;                   // SPLAT_OPT_COUNT_FIRST: 0 only slots without a layout; 1 + the 64 moving frames behind a run of frames that outgrew
                                           // their regions (three in four of the recent ones); 2 + every frame whose camera moved by more than half a degree
    bool idle = false;                     // nothing of this context is in flight (set by the waits that drain every stream, cleared by every enqueue)
    int start_hints = 2;                   // SPLAT_OPT_START_HINTS / SPLAT_START_HINTS: 0 the compositor scans for its walks' starts on every frame; 1 not with
                                           // a camera at rest; 2 nor, three frames of four, with one in slow motion (see enqueue_frame)
    bool one_pass_select = true;           // SPLAT_DBG_ONE_PASS_SELECT=0: near selection always takes its two passes (histogram, compaction)
    int start_refine = 1;                  // SPLAT_OPT_START_REFINE / SPLAT_START_REFINE: a camera at rest refines its walks' starts (splat_policy_decision::refine)
    unsigned int* need_hint = nullptr;     // the per-tile hint table (HintTable of splat_internal.h, m_alloc words a plane: hint_table() below): first in
                                           // it, per tile and wave, the nearest keys its walk needed in the most recent frame
    bool last_near = false;                // the most recent frame ran with near selection: its long lists are unordered in memory
    int timing_every = 8;                  // SPLAT_TIMING_EVERY: per-kernel events on every n-th frame (and whenever stats are asked for)
    int pipeline = 6;                      // frames in flight on the device (SPLAT_PIPELINE = 1..6, see enqueue_frame)
    // Compositor LANES (splat_set_frame_overlap): the compositors of consecutive frames run one after the other on the
    // context's stream (lane 0) -- unless overlap is on and the frames go to DIFFERENT images (a swap chain), in which case
    // the second lane (the copy stream: ensure_lane) takes every other one and two compositors share the chip.  A frame that is
    // bound by the latency of its densest tile's lone wave (small scenes, multi-GPU slabs) leaves the chip mostly idle:
    // with two lanes C2 runs at 7.9 k instead of 5.7 k frames/s, an eighth-of-a-frame slab at 0.08 instead of 0.13 ms.
    // lane[q]: its most recent frame (sequence number, event-ring entry).  img_tab: the most recent frame of every image
    // seen lately (address range, lane, ring entry) -- hazards are decided per IMAGE: with three images in rotation the
    // earlier frame to an image is not its lane's last one.
    struct Lane { uint64_t seq = 0; int ring = -1; };
    Lane lane[2];
    struct ImgRec { const char* lo = nullptr; const char* hi = nullptr; uint64_t seq = 0; int ring = -1; int lane = 0; };
    static constexpr int N_IMG_TAB = 8;
    ImgRec img_tab[N_IMG_TAB];
    hipStream_t comp2 = nullptr;           // lane 1 (lane 0 is `stream`)
    int overlap = 1;                       // splat_set_frame_overlap / SPLAT_FRAME_OVERLAP: 2 = asynchronous frames may use lane 1
    int last_lane = 0;                     // the lane of the most recent frame
    uint64_t lane_seq = 0;
    bool streamed_call = false;            // splat_render_stream is rendering: its frames stay on lane 0 (lane 1's stream carries their copies)
    hipEvent_t pre_wait = nullptr;         // one-shot: the next frame's compositor waits for it (splat_render_stream: its image is still crossing PCIe)
    uint32_t env_pinned = 0;               // bit k: SPLAT_OPT_k was set from the environment at splat_create (splat_set_option leaves it alone)
    int host_zero_copy = 1;                // SPLAT_OPT_HOST_ZERO_COPY: splat_render_frame's compositor stores into a device-addressable host image
    uint64_t region_mult = 0;              // the key buffer's entries per Gaussian chosen for this scene (0: not yet)
    unsigned int keys_per_gaussian = 0;    // SPLAT_OPT_KEYS_PER_GAUSSIAN: 0 = default_region_capacity decides
    splat::CommState* comm = nullptr;      // multi-GPU: RCCL communicator + partition (splat_multi.hip)
    std::string err;
};
#endif
