// splat_internal.h -- shared between the host files (splat_api.hip, splat_scene.hip) and the kernel files (splat_kernels.hip,
// splat_ply.hip, splat_ply_encode.hip, splat_update.hip, splat_select.hip, splat_compact.hip, splat_neighbours.hip, splat_pick.hip,
// splat_colour.hip, splat_visibility.hip).
#ifndef SPLAT_INTERNAL_H
#define SPLAT_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/splat_hip.h"

#ifndef SPLAT_K1X
#define SPLAT_K1X 0      // K1 timing experiments (tools/k1_ab.py); 0 = the product
#endif
// Round-7 timing experiments (tools/lab/build_variant.sh name -DSPLAT_EXP_...=...; profiles/r07_*): 0 = the product
#ifndef SPLAT_EXP_STAGE2
#define SPLAT_EXP_STAGE2 0     // compositor: the staging verdicts computed twice (what they cost)
#endif
#ifndef SPLAT_EXP_NO_BRACKET
#define SPLAT_EXP_NO_BRACKET 0 // compositor, retained frames: hinted exact walks skip the bracket, single-state from 0 (what the bracket costs at rest; invalid frames)
#endif
#ifndef SPLAT_EXP_K1DUMMY
#define SPLAT_EXP_K1DUMMY 0    // K1: this many dummy VALU instructions per (Gaussian, tile) hand-out step (what per-pair verdicts would cost)
#endif
#ifndef SPLAT_EXP_SKIPFULL
#define SPLAT_EXP_SKIPFULL 0   // near selection: lists of this many keys or more that need a full sort are left unsorted (what their sort costs a frame)
#endif
#ifndef SPLAT_EXP_SORT2
#define SPLAT_EXP_SORT2 0      // compositor: the short lists' in-LDS sort run twice (what it costs)
#endif
#ifndef SPLAT_EXP_K1DROP
#define SPLAT_EXP_K1DROP 0     // K1: 1 = close-up rectangles dropped from binning, n >= 2 = every rectangle of more than n tiles (invalid frames)
#endif

struct SplatShBlocks;             // the three sh rotation blocks (splat_sh_math.h)
struct SplatColourMap;            // a 3x4 map of the colour as the sh coefficients take it (splat_colour_math.h)

namespace splat {

constexpr int TILE = SPLAT_TILE;
constexpr int SCENE_PLANES = 16;  // float4 planes per Gaussian (see pack_scene_kernel)
constexpr int LIVE_PLANES = 10;   // planes read per frame at sh_dim <= 27 (160 B / Gaussian)


// Everything a frame's kernels need, passed by value (kernarg -> SGPRs).
struct FrameConst {
    float view[16];
    float proj[16];
    float w, h;
    float htanx, htany, focal;
    float cam[3];
    float lowpass;
    int sh_dim;
    int y_up, sample_half, zclip;
    float zmin, zmax;
    int W, H;              // integer target size
    int tiles_x;           // tiles per row
    int tile_row0;         // slab: first tile row
    int n_tile_rows;       // slab: tile rows in this context
    int row_px0, row_px1;  // slab pixel rows [row_px0, row_px1)
    float early_eps;       // compositor early-out: transmittance below which a pixel stops needing layers; 0 = off
    float close_width;     // the skipped layers' [lo,hi] bracket counts as closed when hi - lo <= this on every channel:
                           // 0 = the exact frame, 2 = SPLAT_MODE_FAST (the walk continues from the bracket's middle: within 1 of exact)
    int early_min;         // shortest list the early-out is tried on
    int early_scan8;       // the transmittance scan gives up after this many eighths of the list
    int prio_len;          // lists >= prio_len / 2x / 4x run at wave priority 1 / 2 / 3
    unsigned int bucket_cap; // one-pass binning: entries of the key buffer the tiles' regions live in (0: two-pass binning with exact lists)
    int corrected;         // SPLAT_MODE_CORRECTED_PROJECTION: J enters transposed (perspective-shear terms kept)
    int cull_blocks;       // K1 skips 256-Gaussian blocks whose bounds cannot reach the slab (needs lowpass > 0)
    int start_hints;       // compositor: the camera is at rest -- a wave's exact walk may start where the previous frame's did (start_hint) instead of scanning for it
    int start_light;       // ... in very slow motion: half the margin on a hinted start, the scan every eighth frame instead of every fourth
    int redo_only;         // K1 as a REDO launch: leaves at once unless the frame's scan flagged a tile that outgrew its region
    int large_tiles;       // one-pass binning: a splat of more tiles than this goes to the frame's large list (bin_large_kernel); 0 = only
                           // the splats wider or taller than K1's 32 x 32-tile window
};

// Upload-time bounds of one K1 block (256 consecutive slots of the Morton-ordered scene): the AABB
// of the finite positions and the largest Frobenius norm of a cov3d (>= its spectral norm).
struct BlockBounds { float lo[3], hi[3], fmax, pad; };

// Device-side frame status, read back once per frame.
struct FrameStatus {
    unsigned long long n_visible;
    unsigned long long n_singular;
    unsigned long long n_pairs;
    unsigned int max_tile_len;
    unsigned int overflow;   // 1: n_pairs > capacity; 2: a tile outgrew its bucket; 3: more long lists than the
                             // sort grids were sized for; 4: the long lists outgrew the second key buffer.  Emit/sort/composite skipped
    unsigned long long n_fallback;   // waves whose early-out bracket did not close (redone in full)
    unsigned long long n_sort_fallback; // tiles whose radix-by-depth order failed the 64-bit check (depth ties): bitonic redo
    unsigned int n_near_tiles;       // tiles whose long list (> 2048 keys) was served by its selected nearest keys (select_near) ...
    unsigned int n_near_fallback;    // ... and those among them that needed the whole list sorted after all
    unsigned int n_large;            // one-pass binning: splats K1 found large this frame (listed for bin_large_kernel, or only counted)
    unsigned int n_window;           // ... and those among them wider or taller than K1's 32 x 32-tile window (one atomic per pair without a list)
    unsigned int n_ge8192, n_ge2048;    // tiles whose list has >= 8192 / >= 2048 keys: in `order` they are a prefix
    unsigned int n_ge16384;             // likewise >= 16384 (the lists sorted as several runs and merged)
    unsigned int redone;                // 1: the frame outgrew its regions and was binned again on the device (overflow redo); written by every scan
    unsigned int n_long_keys;           // one-pass binning: entries of the second key buffer the frame's lists of more than 2048 keys ask for
    unsigned int arrived;               // 1: the frame's scan has written this status (the host zeroes its copy when it enqueues the frame)
    unsigned int n_probe_fail;          // waves whose refinement probe (a shallower start at rest) did not close and walked again from the
                                        // known-good start -- not among n_fallback
    unsigned int pad_;                  // (n_blocks_culled is 8-byte aligned)
    unsigned long long n_blocks_culled; // K1 blocks skipped by the bounds test (filled on the host from the block flags)
    unsigned long long layout_total;    // one-pass binning: key-buffer entries the regions built from this frame ask for (layout_kernel)
};

// 48-byte projected record (3 x float4), stored in SLOT order (the Morton order of the scene planes: K1 writes them
// coalesced, the compositor's gathers are local) and gathered by the compositor through the keys' slot halves.
struct Rec {
    float4 a;   // cx, cy, hx, hy
    float4 b;   // conic a, b, c, opacity
    float4 c;   // r, g, b, power below which alpha < 1/255 for certain
};

// Experiment switches of the launch wrappers (SPLAT_SORT_RADIX_MIN, SPLAT_SCAN_THREADS, SPLAT_DBG_NTILES, SPLAT_COMP_LDS_PAD):
// per context, read from the environment at splat_create.  They travel with every launch: each argument block below that needs
// them points at the launching context's set.
struct LaunchKnobs {
    unsigned int sort_radix_min = 128;     // lists up to this length use the bitonic network
    int scan_threads = 0;                  // 0: by the tile count
    unsigned int dbg_ntiles = 0;           // != 0: composite only the N longest tiles
    unsigned int comp_lds_pad = 0;         // extra dynamic LDS per compositor workgroup (an occupancy cap)
    unsigned int k1_lds_pad = 0;           // SPLAT_K1_LDS_PAD: the same for K1 (lab: how K1's time depends on the blocks resident per CU)
    unsigned int dbg_select_stride = 0;    // SPLAT_DBG_SELECT_STRIDE: slots of the tile order per workgroup of the near selection's launch (default 8)
    unsigned long long dbg_keys2_entries = 0; // SPLAT_DBG_KEYS2_ENTRIES: initial size of a frame slot's second key buffer (tests force its growth)
    int dbg_hint_radius = -1;              // SPLAT_DBG_HINT_RADIUS: the near selection's neighbourhood, in tiles (default: by the camera's motion)
    unsigned int dbg_select_blind = 0;     // SPLAT_DBG_SELECT_BLIND: the near selection ignores what the walks needed last frame (every selection is
                                           // near_cap keys: with a small near_cap the long tiles repair themselves on every binned frame -- tests)
    unsigned int dbg_starts = 0;           // SPLAT_DBG_STARTS: statistics frames record (list length, nearest keys the walk needed) per wave
    unsigned int dbg_bracket_count = 0;    // SPLAT_DBG_BRACKET_COUNT: a statistics frame composited from retained lists reports, as n_iter_scan, the
                                           // (wave, record) steps its walks took with both states of the bracket (a frame of that flavour
                                           // that scans -- start hints off, a margin's scan turn -- reports its scan's steps PLUS those)
    unsigned int dbg_proven_starts = 1;    // SPLAT_DBG_PROVEN_STARTS: 0 retained frames bracket every early-out walk, as binned frames do; 2 a walk that
                                           // takes a proof starts from state 255 instead of 0 (the frame must be the same bytes).  The table
                                           // lives with the kept staging verdicts: SPLAT_DBG_STAGE_CACHE=0 turns both off
    unsigned int dbg_stage_cache = 1;      // SPLAT_DBG_STAGE_CACHE: 0 retained frames keep no staging verdicts (and take no proven starts); 2 the host zeroes the kept masks (not
                                           // their counts) in front of every retained frame of a set after the second -- a frame that reads them
                                           // then stages nothing there and comes out wrong: how a test sees that the path is live
};

// The per-tile hint table, kept from frame to frame: ONE allocation of HINT_WORDS planes of `stride` words (the context's
// m_alloc).  A part of P planes holds P words per tile, tile after tile.  This is the only place that knows where the parts are.
struct HintTable {
    unsigned int* base;     // nullptr: no table (every part is nullptr then)
    size_t stride;          // words per plane

    static constexpr unsigned int NEED_PLANE = 0u, NEED_PLANES = 4u;                                   // per wave: the nearest keys of the list its walk needed
    static constexpr unsigned int DEPTH_PLANE = NEED_PLANE + NEED_PLANES, DEPTH_PLANES = 1u;           // the depth the tile's last near selection began at
    static constexpr unsigned int START_PLANE = DEPTH_PLANE + DEPTH_PLANES, START_PLANES = 4u;         // per wave: where its exact walk started
    static constexpr unsigned int REFINE_PLANE = START_PLANE + START_PLANES, REFINE_PLANES = 4u;       // per wave: the state of its start's refinement at rest
    static constexpr unsigned int HINT_WORDS = 13u;                                                    // planes in all = words per tile
    static_assert(DEPTH_PLANE == 4u && START_PLANE == 5u && REFINE_PLANE == 9u && REFINE_PLANE + REFINE_PLANES == HINT_WORDS,
                  "the four parts tile the table exactly");

    unsigned int* plane(unsigned int k) const { return base ? base + k * stride : nullptr; }
    unsigned int* needs() const { return plane(NEED_PLANE); }
    unsigned int* select_depth() const { return plane(DEPTH_PLANE); }
    unsigned int* starts() const { return plane(START_PLANE); }
    unsigned int* refinement() const { return plane(REFINE_PLANE); }
    size_t words() const { return HINT_WORDS * stride; }
    size_t bytes() const { return sizeof(unsigned int) * words(); }
};

void launch_pack_scene(hipStream_t s, uint64_t n, const float* pos4, const float* cov3d, const float* opacity,
                       const float* sh, const unsigned int* perm, float4* planes);
void launch_cov3d(hipStream_t s, uint64_t n, const float* scales3, const float* rot4, float* cov3d);
// The scene's order on the device (splat_upload_scene_device): orig[j] = the Gaussian stored in slot j, as morton_order of
// splat_scene.hip orders them.  pingpong: 4 n words (the sort's two key and two index arrays); small:
// scene_order_small_bytes(n) bytes (scan tables, partial boxes).  The two events, when given, are recorded around the sort.
size_t scene_order_small_bytes(uint64_t n);
void launch_scene_order(hipStream_t s, uint64_t n, const float* pos4, uint32_t* pingpong, void* small, unsigned int* orig,
                        hipEvent_t sort_begin = nullptr, hipEvent_t sort_end = nullptr);
// ... and the bounds of its K1 blocks, as block_bounds of splat_scene.hip computes them
void launch_block_bounds(hipStream_t s, uint64_t n, const float* pos4, const float* cov3d, const unsigned int* orig, BlockBounds* bounds);

// PLY vertex rows -> the five SoA buffers, activated and recentred as load_from_ply does (splat_ply.hip): decode, the
// sequential sum into mean[3] (device, 3 floats), the subtraction.  ev (nullable): four events recorded around the three.
void launch_ply_decode(hipStream_t s, const splat_ply_layout& lay, const void* d_rows, float* pos4, float* scales3,
                       float* opacity, float* rot4, float* sh, float* mean, hipEvent_t* ev = nullptr);
// how both PLY kernels stage rows in LDS: a workgroup takes min(PLY_ROWS, PLY_STAGE_BYTES / stride) consecutive rows
constexpr unsigned int PLY_ROWS = 256;                         // rows per workgroup at most (and threads per workgroup)
constexpr unsigned int PLY_STAGE_DWORDS = 16384;               // 64 KiB of rows
constexpr unsigned int PLY_STAGE_BYTES = PLY_STAGE_DWORDS * 4 - 8;   // what a run may hold: <= 3 bytes in front of it, the last dword whole
// ... and the way back (splat_ply_encode.hip): the resident scene -> PLY vertex rows, row r = Gaussian r (index == nullptr,
// rows == n) or Gaussian index[r] (checked: launch_index_check), read from slot inv[.] of the planes.  The layout arrives
// checked: stride a multiple of 4 in [4, PLY_STAGE_BYTES], every present offset a multiple of 4 inside the row, no two equal;
// d_rows 4-byte aligned.  Bytes of a row that no slot names are written as 0.
void launch_ply_encode(hipStream_t s, uint64_t n, uint64_t rows, const unsigned int* index, const splat_ply_layout& lay,
                       const unsigned int* inv, const float4* planes, void* d_rows);

// A resident scene edited in place (splat_update.hip).  `fields`: SPLAT_FIELD_* bits; a buffer whose field is not named is
// not read.  The order stays: the whole-field form reads row orig[j] for slot j, the indexed form writes slot
// inv[index[t]] from row t of the compact buffers (inv: launch_inverse_order) and marks the blocks it touched in `dirty`
// (one byte per K1 block, nullptr: not wanted).  launch_index_check adds to *bad the indices that are >= n.
void launch_inverse_order(hipStream_t s, uint64_t n, const unsigned int* orig, unsigned int* inv);
void launch_index_check(hipStream_t s, uint64_t k, uint64_t n, const unsigned int* index, unsigned int* bad);
void launch_repack_scene(hipStream_t s, uint64_t n, uint32_t fields, const float* pos4, const float* cov3d, const float* opacity,
                         const float* sh, const unsigned int* orig, float4* planes);
void launch_repack_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, uint32_t fields, const float* pos4,
                           const float* cov3d, const float* opacity, const float* sh, const unsigned int* inv, float4* planes,
                           unsigned char* dirty);
// ... and the bounds of the K1 blocks from the planes, as block_bounds computes them from the buffers; dirty != nullptr:
// only the blocks whose byte is set, which is cleared
void launch_plane_bounds(hipStream_t s, uint64_t n, const float4* planes, unsigned char* dirty, BlockBounds* bounds);
// ... read back and mapped in place (splat_transform.hip).  The unpacks are the repacks run backwards: the whole-scene form
// writes row orig[j] from slot j, the indexed form row t of the compact buffers from slot inv[index[t]]; pos4's w comes
// back as 1; a buffer whose field is not named is not written.  The transforms apply the 3x4 row-major affine map m to the
// centre and the covariance (splat_transform_math.h) of every slot, or of the slots inv[index[t]], whose blocks are marked
// in `dirty` (required).  The indices arrive checked (launch_index_check).
void launch_unpack_scene(hipStream_t s, uint64_t n, uint32_t fields, float* pos4, float* cov3d, float* opacity, float* sh,
                         const unsigned int* orig, const float4* planes);
void launch_unpack_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, uint32_t fields, float* pos4,
                           float* cov3d, float* opacity, float* sh, const unsigned int* inv, const float4* planes);
void launch_transform_scene(hipStream_t s, uint64_t n, const float m[12], float4* planes);
void launch_transform_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const float m[12],
                              const unsigned int* inv, float4* planes, unsigned char* dirty);
// ... and bands 1-3 of sh turned by the blocks b (splat_sh_math.h) in every slot, or in the slots inv[index[t]]; nothing else
// of a slot changes, so no bounds do
void launch_rotate_sh_scene(hipStream_t s, uint64_t n, const SplatShBlocks& b, float4* planes);
void launch_rotate_sh_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const SplatShBlocks& b,
                              const unsigned int* inv, float4* planes);

// A selection made from the resident scene (splat_select.hip).  SelectView: the camera and conventions the vertex stage's
// geometry half needs -- a frame's, without slab, binning or compositor state.  The query arrives checked, its rectangle
// clamped to the target (x0 > x1 or y0 > y1: empty).  Thread j judges slot j and reads / writes selection[orig[j]]; *count
// (zeroed by the caller) += the Gaussians selected after `op`.
struct SelectView {
    float view[16];
    float proj[16];
    float w, h;
    float htanx, htany, focal;
    float lowpass;
    int y_up, sample_half, zclip;
    float zmin, zmax;
    int W, H;
    int corrected;
};
void launch_select_query(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const splat_select_query& q,
                         const SelectView& v, const unsigned char* pixel_mask, uint32_t op, unsigned char* selection,
                         unsigned int* count);
// ... and its indices: the positions of the nonzero bytes of mask[0..n), ascending, the first `capacity` of them into out.
// counts: selection_groups(mask, n) + 1 words of scratch; the last one receives how many bytes are nonzero.
constexpr unsigned int SELECT_SPAN = 4096;      // bytes of the mask per workgroup, on 16-byte boundaries of the ADDRESS
constexpr unsigned int SELECT_SCAN_ROUND = 256; // workgroup counts the scan takes per round
inline uint64_t selection_groups(const void* mask, uint64_t n) { return (((uintptr_t)mask & 15u) + n + SELECT_SPAN - 1) / SELECT_SPAN; }
void launch_selection_indices(hipStream_t s, uint64_t n, const unsigned char* mask, unsigned int* out, uint64_t capacity,
                              unsigned int* counts);
// (splat_select.hip's scan on its own: counts[0..g) -> their exclusive prefix sums, counts[g] = the total)
void launch_count_scan(hipStream_t s, unsigned int g, unsigned int* counts);
// ... and Gaussians taken out of the scene by one (splat_compact.hip).  launch_index_map: behind launch_selection_indices
// (with no room for indices: the counts and their scan alone) on the same mask, `offsets` the counts it scanned; map[i] (n
// words) = the rank of Gaussian i among the survivors, or REMOVED_INDEX.  launch_compact_scene: the survivors' planes and
// new indices from the scene of n slots to one of n2, slot order kept; block_counts: (n + 255) / 256 + 1 words of scratch.
constexpr unsigned int REMOVED_INDEX = 0xFFFFFFFFu;
void launch_index_map(hipStream_t s, uint64_t n, const unsigned char* mask, const unsigned int* offsets, uint32_t mode,
                      unsigned int* map);
void launch_compact_scene(hipStream_t s, uint64_t n, uint64_t n2, const float4* planes, const unsigned int* orig,
                          const unsigned int* map, unsigned int* block_counts, float4* planes2, unsigned int* orig2);
// ... and Gaussians added to it, and its slots put back in order (splat_append.hip).  launch_grow_scene: the n resident slots'
// planes and indices from stride n to stride n2.  launch_pack_append: behind launch_scene_order of the m new rows into
// orig2 + n; row orig2[n + j] packed into slot n + j of the arrays of n + m slots, orig2[n + j] += n.  launch_order_moved:
// *moved (zeroed by the caller) += the slots j with orig[j] != orig2[j].  launch_permute_scene: slot j of planes2 from slot
// inv[orig2[j]] of planes (inv: launch_inverse_order of the order planes lie in), both of n slots.
void launch_grow_scene(hipStream_t s, uint64_t n, uint64_t n2, const float4* planes, const unsigned int* orig, float4* planes2,
                       unsigned int* orig2);
void launch_pack_append(hipStream_t s, uint64_t n, uint64_t m, const float* pos4, const float* cov3d, const float* opacity,
                        const float* sh, float4* planes2, unsigned int* orig2);
void launch_order_moved(hipStream_t s, uint64_t n, const unsigned int* orig, const unsigned int* orig2, unsigned long long* moved);
void launch_permute_scene(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* inv, const unsigned int* orig2,
                          float4* planes2);
// ... and a selection by neighbourhood (splat_neighbours.hip; r2: the radius squared, finite).  *pairs (zeroed by the caller) +=
// the ordered pairs of K1 blocks whose bounds are within reach of each other.  counts[i] (n words, ORIGINAL index order) =
// min(cap, the Gaussians j != i with source[j] != 0 -- source == nullptr: all -- whose centre is within reach of i's).
// The apply step judges count_min <= counts[i] <= count_max and combines selection[i] as launch_select_query does;
// selection == nullptr: nothing is written and the Gaussians that pass are counted.  *count (zeroed by the caller) += them.
void launch_neighbour_block_pairs(hipStream_t s, uint64_t n, const BlockBounds* bounds, float r2, unsigned long long* pairs);
void launch_neighbour_counts(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const BlockBounds* bounds,
                             const unsigned char* source, float r2, unsigned int cap, unsigned int* counts);
void launch_neighbour_apply(hipStream_t s, uint64_t n, const unsigned int* counts, unsigned int count_min, unsigned int count_max,
                            uint32_t op, unsigned char* selection, unsigned int* count);
// ... and what a pixel is made of (splat_pick.hip).  The query arrives checked; pixels: n_pixels (x, y) pairs in DEVICE memory,
// all on the target, bound: (x0, y0, x1, y1) of all of them; mask: one byte per Gaussian, ORIGINAL index order, or nullptr.
// PickTemps: the call's temporaries -- counts and fronts: n_pixels words each, ZEROED by the caller; list_key and list_alpha:
// n_pixels * max_hits entries each, pixel q's at q * max_hits.  results: n_pixels splat_pick_result; layers: n_pixels *
// max_layers splat_pick_layer (not read when max_layers == 0).  Three launches, each reading what those before it wrote.
constexpr unsigned int PICK_MAX_PIXELS = 256;   // SPLAT_PICK_MAX_PIXELS: the queries fit one workgroup's LDS stage
constexpr unsigned int PICK_MAX_HITS = 4096;    // SPLAT_PICK_MAX_HITS: a pixel's list fits one workgroup's LDS (48 KB)
struct PickTemps {
    unsigned int* counts;
    unsigned long long* fronts;
    unsigned long long* list_key;
    float* list_alpha;
};
void launch_pick(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const unsigned char* mask, const SelectView& v,
                 const splat_pick_query& q, unsigned int n_pixels, const int2* pixels, int4 bound, const PickTemps& t, void* results,
                 void* layers);
// ... and the colour tools (splat_colour.hip, splat_colour_math.h).  The colour of a Gaussian under the camera position
// cam_pos at sh_dim, K1's bit for bit: three floats into row orig[j] of out from slot j, or into row t from slot
// inv[index[t]].  launch_select_colour judges that colour by q (checked) and combines selection[orig[j]] and *count as
// launch_select_query does.  The recolours apply the map m to the sh of every slot, or of the slots inv[index[t]]; nothing
// else of a slot changes, so no bounds do.  The indices arrive checked (launch_index_check).
void launch_eval_colours_scene(hipStream_t s, uint64_t n, const float cam_pos[3], int sh_dim, const unsigned int* orig,
                               const float4* planes, float* out);
void launch_eval_colours_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const float cam_pos[3], int sh_dim,
                                 const unsigned int* inv, const float4* planes, float* out);
void launch_select_colour(hipStream_t s, uint64_t n, const float4* planes, const unsigned int* orig, const splat_colour_query& q,
                          const float cam_pos[3], int sh_dim, uint32_t op, unsigned char* selection, unsigned int* count);
void launch_recolour_scene(hipStream_t s, uint64_t n, const SplatColourMap& m, float4* planes);
void launch_recolour_indexed(hipStream_t s, uint64_t n, uint64_t k, const unsigned int* index, const SplatColourMap& m,
                             const unsigned int* inv, float4* planes);

// ---- The per-frame launches take one argument block each, by const&.  The blocks are plain aggregates without defaults: a
// caller value-initialises one (`ScanArgs a{};`) and what it does not set is zero / nullptr / false.  What travels together
// is a sub-struct:
struct SceneArgs {                  // the uploaded scene
    uint64_t n;
    const float4* planes;
    const unsigned int* orig;       // slot -> original index: the order among equal depths
    const BlockBounds* bounds;
};
struct TileLists {                  // a frame slot's tile lists
    unsigned int *offsets, *order, *lens;   // per tile: where its list starts in keys; the tiles, longest list first; the lists' lengths
    unsigned int* cursor;           // two-pass binning: the emit's cursors
    unsigned int* off2;             // one-pass binning: per tile, where its room in the SECOND key buffer starts -- handed out by the scan to the
                                    // lists of more than 2048 keys; nullptr: at offsets[tile], like its list in keys
    unsigned int* near_m;           // near selection: per tile, how many of the nearest keys are in order
};
struct BinTarget {                  // what K1 bins into
    unsigned int* cursors;          // per tile: pair count (two-pass counting) / cursor of the tile's region
    unsigned int* layout;           // one-pass binning (fc.bucket_cap != 0): cursors[t] is the cursor of tile t's region
                                    // keys[layout[t] .. layout[t+1]); nullptr: two-pass counting
};
struct KeyBuffers {
    unsigned long long *keys, *keys2;   // keys2: sorted near selections, scatter space of the long lists' sorts and merges
    unsigned long long cap;         // entries of keys: beyond it a two-pass frame is flagged (overflow 1)
    unsigned int cap2;              // entries of keys2: beyond it the frame is flagged (overflow 4)
};
struct LargeList {                  // one-pass binning: the frame's list of large splats -- launch_bin_large behind K1 bins them
    uint4* list;                    // nullptr with a counter: large splats are only counted
    unsigned int* count;
    unsigned int cap;               // entries of list
};
struct SortGrids { unsigned int big, mid, lng; };    // how many entries of `order` (longest lists first) the 1024-thread, the 512-thread and the
                                                     // run-merging sort launches cover; the scan validates them against the frame's actual list lengths

// K1, and behind it on the same stream the large splats it listed, tile by tile (bin_large_kernel): both take this block
struct BinArgs {
    hipStream_t s; const LaunchKnobs* knobs; SceneArgs scene; FrameConst fc;
    Rec* recs; float* depth; ushort4* rect; unsigned int* vislist; unsigned long long* keys; FrameStatus* status;
    BinTarget bin;
    unsigned int* blockinfo;        // per block: bit 31 = skipped by culling; one-pass binning: visible | singular << 9
    bool count_only;                // one-pass binning's COUNT flavour: cursors[t] += the tile's pairs and nothing else (no SH, no record,
                                    // no key) -- the pass in front of a layout that fits exactly this camera
    LargeList large;
};
void launch_preprocess(const BinArgs& a);
void launch_bin_large(const BinArgs& a);

struct NextRegions {                // the scan's second workgroup: with both of `to` given it builds the regions + cursors of the next frame on
    BinTarget to;                   // this stream (see launch_layout)
    unsigned int tiles_x, motion_radius;    // != 0 (a moving camera): those regions are sized from the longest list within this many tiles
};                                          // of each tile (build_layout)
struct ScanArgs {
    hipStream_t s; const LaunchKnobs* knobs; unsigned int m;
    BinTarget bin;                  // what the frame was binned into
    TileLists lists; KeyBuffers keys; unsigned int bucket_cap; SortGrids grids; FrameStatus* status;
    FrameStatus* host_status;       // pinned, device-visible: the scan also delivers the status there
    NextRegions next;
    float spare_max;                // how far a region may grow into the buffer's spare room
    bool redo_only;                 // the second scan of a frame binned again on the device: nothing unless status->overflow == 2
    unsigned int* large_count;      // the frame's large-splat counter: reset here for the slot's next K1
};
void launch_scan(const ScanArgs& a);

// the regions (and cursors) of the slot's next one-pass frame from this frame's lists; an all-zero `from.layout` with cursors
// counted from zero is the bootstrap
struct LayoutArgs {
    hipStream_t s; unsigned int m; BinTarget from, next; unsigned int key_entries; FrameStatus *status, *host_status; float spare_max;
    const FrameStatus* redo_gate;   // != nullptr: a redo launch -- does nothing unless redo_gate->overflow == 2
    unsigned int* large_count;      // see ScanArgs
};
void launch_layout(const LayoutArgs& a);

struct EmitArgs {
    hipStream_t s; SceneArgs scene; FrameConst fc; const float* depth; const ushort4* rect; const unsigned int* vislist;
    unsigned int* cursor; unsigned long long* keys; const FrameStatus* status;
};
void launch_emit(const EmitArgs& a);

struct SortArgs {
    hipStream_t s; const LaunchKnobs* knobs; unsigned int n_tiles; SortGrids grids; TileLists lists; KeyBuffers keys; FrameStatus* status;
    const unsigned int* orig;
    unsigned int fused_sort_max;    // lists of up to this many keys (<= 2048) are sorted by the compositor's workgroups themselves
                                    // (launch_composite must be given the same value; launch_sort then leaves them alone); 0 = off
};
void launch_sort(const SortArgs& a);

// near selection instead of the sort launches: the nearest keys of every list of more than 2048 keys, by last frame's need
struct SelectArgs {
    hipStream_t s; const LaunchKnobs* knobs; unsigned int n_tiles; TileLists lists; KeyBuffers keys; FrameStatus* status;
    const unsigned int* orig;
    unsigned int near_cap;
    const unsigned int* need_hint;  // HintTable::needs()
    unsigned int* near_thr;         // HintTable::select_depth(); nullptr: every selection takes its two passes
    unsigned int tiles_x, tile_rows;    // the tile grid: a tile's selection also looks at its neighbours' hints
    unsigned int grid;              // workgroups (each strides over the tile order); 0 = an eighth of the tiles
    bool at_rest;                   // the camera of the last frames: selections sized tightly
    int hint_radius;                // a tile's selection is sized from its own walks' need and its neighbours' within this many tiles
};
void launch_select(const SelectArgs& a);

struct CompositeArgs {
    hipStream_t s; const LaunchKnobs* knobs; unsigned int n_tiles; FrameConst fc;
    TileLists lists;                // near_m != nullptr (with keys2): near selection -- launch_select ran in front: of a list of more than
                                    // 2048 keys only the nearest near_m[tile] are in order (composite_tile)
    KeyBuffers keys;                // keys2 != nullptr: no sort launch ran; lists of more than 2048 keys are sorted by their tile's
                                    // workgroup through this buffer
    const Rec* recs; uint32_t* argb; FrameStatus* status; const unsigned int* orig;
    unsigned int fused_sort_max;    // see SortArgs
    uint2* iters;                   // per wave (scan, blend) iteration counts, statistics frames only
    bool keep_keys;                 // lists sorted inside the compositor are also written back to the bucket (the debug getters
                                    // read them there); off on ordinary frames
    bool pair_walk;                 // the two-records-per-step flavour of the exact walk (same pixels)
    bool libm_exp;                  // SPLAT_MODE_LIBM_EXP: expf as the host libm computes it
    bool clear_first;               // the frame starts from a cleared image: old pixels are not read, tiles nothing covers are zeroed
                                    // (color.clear(0) of src/main.rs:73, fused)
    HintTable hints;                // needs(): how many of its list's nearest keys each wave's walk needed (sizes the next frame's selection);
                                    // starts(): where each wave's exact walk started, in keys from the list's near end (fc.start_hints);
                                    // refinement(): each wave's start refinement at rest (composite_tile, phase A)
    unsigned int refine;            // != 0: this frame's waves refine their starts (splat_policy_decision::refine)
    unsigned int* proven_start;     // ... and the starts its set has proven (CompArgs::proven_start); nullptr: none
    unsigned int* stage_nv;         // a frame composited from retained lists: the staging verdicts its walks take from the frames before it
    unsigned long long* stage_mask; // and leave for the next -- 4 words / 4 x 32 masks per tile (CompArgs); nullptr: none kept
};
void launch_composite(const CompositeArgs& a);

// What each Gaussian contributes to a view (splat_visibility.hip), behind K1's counting flavour, the scan, the emit and the sort
// launches of a two-pass binning over the WHOLE target with every list in order: offsets / lens / keys are its tile lists (keys
// carry slots, blend order: a list's far end is the nearest), recs / rect its records and covered rectangles in slot order.
// The region arrives checked: x0 <= x1 and y0 <= y1 inside the target, or empty (nothing is launched); pixel_mask: W * H bytes
// or nullptr; mask: one byte per Gaussian, ORIGINAL index order, or nullptr.  The three outputs (n entries each, ORIGINAL index
// order, each nullable) are ADDED to (pixels, weight_sum) and MAXED (max_weight, by its bits): the caller zeroes them for a SET.
struct VisibilityArgs {
    hipStream_t s; int W, tiles_x, y_up, sample_half;
    int x0, y0, x1, y1; float weight_min;
    const unsigned int *offsets, *lens; const unsigned long long* keys; const Rec* recs; const ushort4* rect; const unsigned int* orig;
    const unsigned char *mask, *pixel_mask;
    unsigned int* pixels; float* max_weight; unsigned long long* weight_sum;
};
void launch_visibility(const VisibilityArgs& a);
// a frame composited from retained lists: its device status starts from these values (no scan ran to initialise it)
void launch_status_set(hipStream_t s, FrameStatus* status, const FrameStatus& v);
hipError_t init_device_kernels();   // per-device kernel attributes; call with the device current

// ---- splat_multi.hip: the multi-GPU layer's hooks into a context (splat_ctx itself stays private to the host files that
// include splat_context.h: splat_api.hip, splat_scene.hip)
struct CommState;                              // RCCL communicator + partition of one context
CommState** ctx_comm_slot(splat_ctx* c);
hipStream_t ctx_stream(splat_ctx* c);
hipStream_t frame_stream(splat_ctx* c);    // the stream the most recent frame's compositor is on (compositor lanes, splat_api.hip)
int ctx_device(const splat_ctx* c);
int frame_tail(splat_ctx* c);                // re-record the most recent frame's "ended" event behind work enqueued on its lane (a row gather)
int ctx_quiesce(splat_ctx* c);               // wait for everything enqueued; a skipped frame stays pending for splat_sync
int ctx_fail(splat_ctx* c, int code, const char* msg);
void comm_release(CommState* s);               // splat_destroy -> here

}  // namespace splat
#endif
