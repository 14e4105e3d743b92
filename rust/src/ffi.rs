//! `extern "C"` view of include/splat_hip.h -- field for field, in declaration order.
//! UNTESTED here (no rustc in the authoring image); tests/test_host.py checks the same header against the
//! ctypes binding, and examples/render_c.c compiles it as C99.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

pub const SPLAT_OK: c_int = 0;
pub const SPLAT_ERR_INVALID: c_int = -1;
pub const SPLAT_ERR_HIP: c_int = -2;
pub const SPLAT_ERR_NO_SCENE: c_int = -3;
pub const SPLAT_ERR_CAPACITY: c_int = -4;
pub const SPLAT_MODE_EXACT: i32 = 0;
pub const SPLAT_MODE_CORRECTED_PROJECTION: i32 = 1;
pub const SPLAT_MODE_LIBM_EXP: i32 = 2;
pub const SPLAT_MODE_FAST: i32 = 4;
// the fields an in-place edit names (splat_update_scene_device, splat_update_gaussians_device)
pub const SPLAT_FIELD_POS: u32 = 1;
pub const SPLAT_FIELD_COV3D: u32 = 2;
pub const SPLAT_FIELD_OPACITY: u32 = 4;
pub const SPLAT_FIELD_SH: u32 = 8;
// the tests a selection query names, and how its result combines with the selection (splat_select_device)
pub const SPLAT_SEL_VOLUME: u32 = 1;
pub const SPLAT_SEL_SCREEN: u32 = 2;
pub const SPLAT_SEL_DEPTH: u32 = 4;
pub const SPLAT_SEL_OPACITY: u32 = 8;
pub const SPLAT_SEL_OP_SET: u32 = 0;
pub const SPLAT_SEL_OP_ADD: u32 = 1;
pub const SPLAT_SEL_OP_SUBTRACT: u32 = 2;
pub const SPLAT_SEL_OP_INTERSECT: u32 = 3;
// tuning options (splat_set_option / splat_get_option): equivalent schedules and storage sizes, never pixels
pub const SPLAT_OPT_PIPELINE_DEPTH: i32 = 1;
pub const SPLAT_OPT_FUSED_SORT_MAX: i32 = 2;
pub const SPLAT_OPT_REGION_SPARE: i32 = 3;
pub const SPLAT_OPT_EARLY_OUT_EPS: i32 = 4;
pub const SPLAT_OPT_EARLY_OUT_MIN_LIST: i32 = 5;
pub const SPLAT_OPT_EARLY_OUT_SCAN_EIGHTHS: i32 = 6;
pub const SPLAT_OPT_SORT_IN_COMPOSITOR: i32 = 7;
pub const SPLAT_OPT_PAIR_WALK: i32 = 8;
pub const SPLAT_OPT_TIMING_EVERY: i32 = 9;
pub const SPLAT_OPT_BLOCK_CULLING: i32 = 10;
pub const SPLAT_OPT_ONE_PASS_BINNING: i32 = 11;
pub const SPLAT_OPT_KEY_BUFFER_BYTES: i32 = 12;
pub const SPLAT_OPT_FAST_CLOSE_WIDTH: i32 = 13;
pub const SPLAT_OPT_PRIORITY_LIST_LEN: i32 = 14;
pub const SPLAT_OPT_FRAME_OVERLAP: i32 = 15;
pub const SPLAT_OPT_NEAR_SELECT_KEYS: i32 = 16;
pub const SPLAT_OPT_OVERFLOW_REDO: i32 = 17;
pub const SPLAT_OPT_START_HINTS: i32 = 18;
pub const SPLAT_OPT_HOST_ZERO_COPY: i32 = 19;
pub const SPLAT_OPT_KEYS_PER_GAUSSIAN: i32 = 20;
pub const SPLAT_OPT_COUNT_FIRST: i32 = 21;
pub const SPLAT_OPT_LARGE_SPLAT_TILES: i32 = 22;
pub const SPLAT_OPT_LARGE_LIST_MIN: i32 = 23;
pub const SPLAT_OPT_START_REFINE: i32 = 24;
pub const SPLAT_OPT_RETAIN_LISTS: i32 = 25;
/// SPLAT_ABI_VERSION of the header this file mirrors; compared with splat_abi_version() before the first call
pub const SPLAT_ABI_VERSION: u32 = 7;

#[repr(C)] pub struct SplatCtx { _private: [u8; 0] }
#[repr(C)] pub struct SplatMulti { _private: [u8; 0] }

#[repr(C)] #[derive(Clone, Copy)]
pub struct SplatConfig {
    pub device: i32, pub mode: i32,
    pub y_up: i32, pub sample_half: i32, pub zclip: i32, pub zmin: f32, pub zmax: f32,
    pub pair_capacity: u64,
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct SplatCamera {
    pub view: [f32; 16], pub proj: [f32; 16],      // nalgebra as_slice(): column-major
    pub w: f32, pub h: f32,
    pub htanx: f32, pub htany: f32, pub focal: f32,
    pub cam_pos: [f32; 3],
    pub lowpass: f32, pub sh_dim: i32,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatStats {
    pub n_gaussians: u64, pub n_visible: u64, pub n_singular: u64, pub n_pairs: u64,
    pub max_tile_len: u64, pub bytes_algorithmic: u64,
    pub ms_preprocess: f32, pub ms_scan: f32, pub ms_emit: f32, pub ms_sort: f32,
    pub ms_composite: f32, pub ms_total: f32,
    pub n_fallback: u64, pub n_sort_fallback: u64, pub n_iter_scan: u64, pub n_iter_blend: u64,
    pub n_blocks_culled: u64, pub flops_algorithmic: u64,
    pub n_near_tiles: u64, pub n_near_fallback: u64,
}

pub const SPLAT_PLY_SLOTS: usize = 59;
// where in a vertex row the float32 property feeding each destination slot lies (-1 = absent); slots: 0-2 x y z,
// 3-5 scale_0..2, 6 opacity, 7-10 rot_1 rot_2 rot_3 rot_0, 11-13 f_dc_0..2, 14-58 f_rest_0..44
#[repr(C)] #[derive(Clone, Copy)]
pub struct SplatPlyLayout {
    pub n: u64, pub stride: u32, pub offset: [i32; SPLAT_PLY_SLOTS],
}

// the visibility query: what it does with the output arrays, and its 24-byte layout
pub const SPLAT_VIS_SET: u32 = 0;
pub const SPLAT_VIS_ACCUMULATE: u32 = 1;
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatVisibilityQuery {
    pub weight_min: f32,                           // a hit is seen when its weight is at least this; in [0, 1)
    pub x0: i32, pub y0: i32, pub x1: i32, pub y1: i32,    // the region's rectangle, inclusive; clamped to the target
    pub op: u32,                                   // SPLAT_VIS_*
}

// the pick: its limits, the index of "none", the one flag of a result, and the three layouts (16, 32 and 16 bytes)
pub const SPLAT_PICK_MAX_PIXELS: u32 = 256;
pub const SPLAT_PICK_MAX_HITS: u32 = 4096;
pub const SPLAT_PICK_NONE: u32 = 0xFFFF_FFFF;
pub const SPLAT_PICK_TRUNCATED: u32 = 1;
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatPickQuery {
    pub alpha_min: f32,                            // a hit's alpha is at least this
    pub coverage_min: f32,                         // the surface: the first hit whose coverage reaches this; in (0, 1]
    pub max_hits: u32,                             // the list kept per pixel: 1 ..= SPLAT_PICK_MAX_HITS
    pub max_layers: u32,                           // layer rows per pixel; 0 = none; <= max_hits
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatPickResult {
    pub n_hits: u32, pub flags: u32, pub front_index: u32,
    pub front_depth: f32, pub front_alpha: f32,
    pub surface_index: u32,
    pub surface_depth: f32, pub surface_coverage: f32,
}
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatPickLayer {
    pub index: u32,
    pub depth: f32, pub alpha: f32, pub coverage: f32,
}

// splat_remove_gaussians_device's mode: which side of the selection goes
pub const SPLAT_REMOVE_SELECTED: u32 = 0;
pub const SPLAT_REMOVE_UNSELECTED: u32 = 1;

// a selection query: a Gaussian passes when every test named in `tests` (SPLAT_SEL_* bits) passes; 0 = all pass
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatSelectQuery {
    pub tests: u32,
    pub volume_shape: u32,                         // 0 = box, 1 = ellipsoid
    pub world_to_unit: [f32; 12],                  // 3x4 row-major affine map, world -> the unit shape
    pub screen_rule: u32,                          // 0 = centre, 1 = touch
    pub x0: i32, pub y0: i32, pub x1: i32, pub y1: i32,    // inclusive pixel rectangle
    pub depth_min: f32, pub depth_max: f32,
    pub opacity_min: f32, pub opacity_max: f32,
}

// a colour query (splat_select_colour_device): a Gaussian passes when colour_to_unit maps the colour it is drawn with into the
// unit box / ball -- the VOLUME test's semantics in colour space
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatColourQuery {
    pub colour_to_unit: [f32; 12],                 // 3x4 row-major affine map, colour -> the unit shape
    pub shape: u32,                                // 0 = box, 1 = ellipsoid
    pub clamp: u32,                                // nonzero: the colour is clamped to [0, 1] per channel before the map
}

#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct SplatRecord {
    pub cx: f32, pub cy: f32, pub hx: f32, pub hy: f32,
    pub conic_a: f32, pub conic_b: f32, pub conic_c: f32, pub opacity: f32,
    pub r: f32, pub g: f32, pub b: f32, pub depth: f32,
    pub px0: i32, pub px1: i32, pub py0: i32, pub py1: i32,
}

extern "C" {
    pub fn splat_abi_version() -> u32;
    pub fn splat_stats_size() -> u64;
    pub fn splat_default_config(cfg: *mut SplatConfig);
    pub fn splat_create(cfg: *const SplatConfig, out: *mut *mut SplatCtx) -> c_int;
    pub fn splat_destroy(ctx: *mut SplatCtx);
    pub fn splat_last_error(ctx: *const SplatCtx) -> *const c_char;
    pub fn splat_upload_scene(ctx: *mut SplatCtx, n: u64, pos4: *const f32, cov3d: *const f32,
                              opacity: *const f32, sh: *const f32) -> c_int;
    pub fn splat_compute_cov3d(ctx: *mut SplatCtx, n: u64, scales3: *const f32, rot4: *const f32,
                               cov3d_out: *mut f32) -> c_int;
    // the scene from DEVICE buffers of the context's GPU (same layouts); producer_stream: the hipStream_t that wrote them, or null
    pub fn splat_upload_scene_device(ctx: *mut SplatCtx, n: u64, d_pos4: *const c_void, d_cov3d: *const c_void,
                                     d_opacity: *const c_void, d_sh: *const c_void, producer_stream: *mut c_void) -> c_int;
    pub fn splat_compute_cov3d_device(ctx: *mut SplatCtx, n: u64, d_scales3: *const c_void, d_rot4: *const c_void,
                                      d_cov3d_out: *mut c_void, producer_stream: *mut c_void) -> c_int;
    // the scene from PLY vertex rows in DEVICE memory: decoded, activated and recentred as load_from_ply does, on the GPU
    // (added under ABI version 7: a library of that version may predate them -- look them up by symbol where that matters)
    pub fn splat_decode_ply_device(ctx: *mut SplatCtx, layout: *const SplatPlyLayout, d_rows: *const c_void, d_pos4: *mut c_void,
                                   d_scales3: *mut c_void, d_opacity: *mut c_void, d_rot4: *mut c_void, d_sh: *mut c_void,
                                   producer_stream: *mut c_void) -> c_int;
    pub fn splat_upload_ply_device(ctx: *mut SplatCtx, layout: *const SplatPlyLayout, d_rows: *const c_void, compute_cov3d: i32,
                                   producer_stream: *mut c_void) -> c_int;
    // the way back (added under ABI 7, found by symbol like the two above): the resident scene as PLY vertex rows in DEVICE
    // memory -- log scales and a quaternion from cov3d, the logit of the opacity, positions and sh with their bits; everything
    // that places a float (d_rows_out, stride, present offsets) a multiple of 4, stride <= 65528; row t = Gaussian t, or d_index[t]
    pub fn splat_encode_ply_scene_device(ctx: *mut SplatCtx, layout: *const SplatPlyLayout, d_rows_out: *mut c_void) -> c_int;
    pub fn splat_encode_ply_gaussians_device(ctx: *mut SplatCtx, k: u64, d_index: *const c_void, layout: *const SplatPlyLayout,
                                             d_rows_out: *mut c_void, producer_stream: *mut c_void) -> c_int;
    // the resident scene edited in place, n fixed (added under ABI 7, found by symbol like the two above): `fields` = SPLAT_FIELD_*
    // bits, a buffer whose field is not named may be null; the indexed form takes k compact rows, row t for Gaussian d_index[t]
    pub fn splat_update_scene_device(ctx: *mut SplatCtx, n: u64, fields: u32, d_pos4: *const c_void, d_cov3d: *const c_void,
                                     d_opacity: *const c_void, d_sh: *const c_void, producer_stream: *mut c_void) -> c_int;
    pub fn splat_update_gaussians_device(ctx: *mut SplatCtx, k: u64, d_index: *const c_void, fields: u32, d_pos4: *const c_void,
                                         d_cov3d: *const c_void, d_opacity: *const c_void, d_sh: *const c_void,
                                         producer_stream: *mut c_void) -> c_int;
    // a selection made on the GPU from the resident scene (added under ABI 7, found by symbol like those above): d_selection = one
    // byte per Gaussian in device memory, original index order, nonzero = selected; cam may be null unless SCREEN or DEPTH is
    // named, d_pixel_mask (w*h u8, centre rule only) and count_out may be null; op = SPLAT_SEL_OP_*
    pub fn splat_select_device(ctx: *mut SplatCtx, q: *const SplatSelectQuery, cam: *const SplatCamera, d_pixel_mask: *const c_void,
                               op: u32, d_selection: *mut c_void, count_out: *mut u64, producer_stream: *mut c_void) -> c_int;
    // ... and its indices, ascending, as u32: a d_index for splat_update_gaussians_device; *count_out may exceed capacity
    pub fn splat_selection_indices_device(ctx: *mut SplatCtx, n: u64, d_selection: *const c_void, d_index_out: *mut c_void,
                                          capacity: u64, count_out: *mut u64, producer_stream: *mut c_void) -> c_int;
    // ... and a selection by neighbourhood (added under ABI 7, found by symbol): Gaussian i passes when the other Gaussians of the
    // source set (d_source: n bytes, null = all; may be d_selection itself) within `radius` of its centre number count_min ..=
    // count_max; d_counts_out (n u32) and d_selection may be null, not both; max_block_pairs bounds the work (0 = no limit,
    // beyond it SPLAT_ERR_CAPACITY with nothing written); block_pairs_out and count_out may be null
    pub fn splat_select_neighbours_device(ctx: *mut SplatCtx, radius: f32, d_source: *const c_void, count_min: u32, count_max: u32,
                                          op: u32, d_selection: *mut c_void, d_counts_out: *mut c_void, max_block_pairs: u64,
                                          block_pairs_out: *mut u64, count_out: *mut u64, producer_stream: *mut c_void) -> c_int;
    // ... and the pick (added under ABI 7, found by symbol): the Gaussians whose fragment the reference accepts at up to
    // SPLAT_PICK_MAX_PIXELS pixels of the target of cam (pixels_xy: n_pixels (x, y) pairs in HOST memory), nearest first; per pixel
    // a SplatPickResult into d_results and, with max_layers > 0, max_layers SplatPickLayer rows into d_layers (device memory;
    // d_layers may be null when max_layers == 0); d_mask: one byte per Gaussian like a selection, null = all
    pub fn splat_pick_device(ctx: *mut SplatCtx, q: *const SplatPickQuery, cam: *const SplatCamera, n_pixels: u32,
                             pixels_xy: *const i32, d_mask: *const c_void, d_results: *mut c_void, d_layers: *mut c_void,
                             producer_stream: *mut c_void) -> c_int;
    // ... and the visibility query (added under ABI 7, found by symbol): per Gaussian, on how many pixels of the region of cam's
    // target it is SEEN (weight T * alpha >= weight_min on the pick's hit list, nearest first), its greatest weight and the Q24
    // sum of its weights, into d_pixels (n u32), d_max_weight (n f32), d_weight_sum (n u64): device memory, each may be null, not
    // all; d_pixel_mask (w * h bytes) and d_mask (n bytes like a selection) may be null; q.op: SPLAT_VIS_SET zeroes first,
    // SPLAT_VIS_ACCUMULATE adds and maxes on top -- a loop over cameras
    pub fn splat_visibility_device(ctx: *mut SplatCtx, q: *const SplatVisibilityQuery, cam: *const SplatCamera,
                                   d_pixel_mask: *const c_void, d_mask: *const c_void, d_pixels: *mut c_void,
                                   d_max_weight: *mut c_void, d_weight_sum: *mut c_void, producer_stream: *mut c_void) -> c_int;
    // ... and counts turned into a selection: Gaussian i passes when count_min <= d_counts[i] <= count_max (n u32 in device
    // memory), combined with d_selection (n bytes) by op = SPLAT_SEL_OP_*; needs no scene; count_out may be null
    pub fn splat_select_counts_device(ctx: *mut SplatCtx, n: u64, d_counts: *const c_void, count_min: u32, count_max: u32, op: u32,
                                      d_selection: *mut c_void, count_out: *mut u64, producer_stream: *mut c_void) -> c_int;
    // ... and Gaussians taken out of the scene by a selection (added under ABI 7, found by symbol): mode = SPLAT_REMOVE_*;
    // d_selection = n bytes like a selection, n the resident scene's; *n_out (required) = the survivors, renumbered by their rank
    // in original index order; d_index_map_out (n u32, may be null): the new index of every old Gaussian, or 0xFFFF_FFFF
    pub fn splat_remove_gaussians_device(ctx: *mut SplatCtx, n: u64, d_selection: *const c_void, mode: u32,
                                         d_index_map_out: *mut c_void, n_out: *mut u64, producer_stream: *mut c_void) -> c_int;
    // ... and Gaussians added to it (added under ABI 7, found by symbol): m rows in splat_upload_scene_device's four device
    // buffers, n the resident scene's; *n_out (required) = n + m; the new rows get the original indices n .. n+m-1 and are
    // ordered among themselves behind the resident slots, which stay.  No scene: SPLAT_ERR_NO_SCENE (that takes an upload)
    pub fn splat_append_gaussians_device(ctx: *mut SplatCtx, n: u64, m: u64, d_pos4: *const c_void, d_cov3d: *const c_void,
                                         d_opacity: *const c_void, d_sh: *const c_void, n_out: *mut u64,
                                         producer_stream: *mut c_void) -> c_int;
    // ... and its slots put into the order a fresh upload of its current values would have; *moved_out (may be null) = the
    // slots that hold another Gaussian than before, 0: the call has been a read
    pub fn splat_reorder_scene_device(ctx: *mut SplatCtx, moved_out: *mut u64) -> c_int;
    // the resident values given back, and mapped where they lie (added under ABI 7, found by symbol like those above): the reads
    // are the updates' inverses (same layouts and SPLAT_FIELD_* bits; pos4 gets w = 1; a buffer whose field is not named may be
    // null and is left untouched) and read the scene as a selection does; m = 3x4 row-major affine map in HOST memory, applied
    // to positions and 3D covariances (A S A^T) in place -- an edit like the updates; sh is not rotated
    pub fn splat_read_scene_device(ctx: *mut SplatCtx, n: u64, fields: u32, d_pos4: *mut c_void, d_cov3d: *mut c_void,
                                   d_opacity: *mut c_void, d_sh: *mut c_void) -> c_int;
    pub fn splat_read_gaussians_device(ctx: *mut SplatCtx, k: u64, d_index: *const c_void, fields: u32, d_pos4: *mut c_void,
                                       d_cov3d: *mut c_void, d_opacity: *mut c_void, d_sh: *mut c_void,
                                       producer_stream: *mut c_void) -> c_int;
    pub fn splat_transform_scene_device(ctx: *mut SplatCtx, m: *const f32) -> c_int;
    pub fn splat_transform_gaussians_device(ctx: *mut SplatCtx, k: u64, d_index: *const c_void, m: *const f32,
                                            producer_stream: *mut c_void) -> c_int;
    // view-dependent colour turned with the scene (added under ABI 7, found by symbol): r = 3x3 row-major ORTHOGONAL map in HOST
    // memory (max |R R^T - I| <= 1e-4, else SPLAT_ERR_INVALID; a reflection is fine); bands 1-3 of sh are multiplied by the
    // blocks the first call returns (host only, no context: d1 3x3, d2 5x5, d3 7x7, row-major) -- an edit like an update of sh
    pub fn splat_sh_rotation_blocks(r: *const f32, d1: *mut f32, d2: *mut f32, d3: *mut f32) -> c_int;
    pub fn splat_rotate_sh_scene_device(ctx: *mut SplatCtx, r: *const f32) -> c_int;
    pub fn splat_rotate_sh_gaussians_device(ctx: *mut SplatCtx, k: u64, d_index: *const c_void, r: *const f32,
                                            producer_stream: *mut c_void) -> c_int;
    // colour (added under ABI 7, found by symbol): the colour every Gaussian (d_index null, k == n, original order) or Gaussian
    // d_index[t] is drawn with under cam (cam_pos and sh_dim alone are read) -- K1's rgb bit for bit, unclamped, three f32 a row
    // into d_rgb_out; a selection by that colour (op = SPLAT_SEL_OP_*, count_out may be null); and rgb' = A rgb + t (m = 3x4
    // row-major in HOST memory, every entry finite) applied to the sh coefficients in place -- an edit like an update of sh
    pub fn splat_eval_colours_device(ctx: *mut SplatCtx, cam: *const SplatCamera, k: u64, d_index: *const c_void, d_rgb_out: *mut c_void,
                                     producer_stream: *mut c_void) -> c_int;
    pub fn splat_select_colour_device(ctx: *mut SplatCtx, q: *const SplatColourQuery, cam: *const SplatCamera, op: u32,
                                      d_selection: *mut c_void, count_out: *mut u64, producer_stream: *mut c_void) -> c_int;
    pub fn splat_recolour_scene_device(ctx: *mut SplatCtx, m: *const f32) -> c_int;
    pub fn splat_recolour_gaussians_device(ctx: *mut SplatCtx, k: u64, d_index: *const c_void, m: *const f32,
                                           producer_stream: *mut c_void) -> c_int;
    // debug / stage parity: the stored order (n u32) and the K1 block bounds (ceil(n/256) x 8 f32); either may be null
    pub fn splat_get_scene_layout(ctx: *mut SplatCtx, orig_out: *mut u32, n: u64, bounds_out: *mut f32, n_blocks: u64) -> c_int;
    pub fn splat_set_slab(ctx: *mut SplatCtx, tile_row0: i32, tile_row1: i32) -> c_int;
    pub fn splat_tile_row_loads(ctx: *mut SplatCtx, cam: *const SplatCamera, row_pairs: *mut u64, n_rows: i32) -> c_int;
    pub fn splat_render(ctx: *mut SplatCtx, cam: *const SplatCamera, argb: *mut u32, stats: *mut SplatStats) -> c_int;
    // `color.clear(0); render_to_buffer(&mut color)` (src/main.rs:73-74) in one call: argb_out is written, never read
    pub fn splat_render_frame(ctx: *mut SplatCtx, cam: *const SplatCamera, argb_out: *mut u32, stats: *mut SplatStats) -> c_int;
    pub fn splat_render_device(ctx: *mut SplatCtx, cam: *const SplatCamera, d_argb: *mut c_void,
                               sync: i32, stats: *mut SplatStats) -> c_int;
    pub fn splat_render_frame_device(ctx: *mut SplatCtx, cam: *const SplatCamera, d_argb: *mut c_void,
                                     sync: i32, stats: *mut SplatStats) -> c_int;
    pub fn splat_sync(ctx: *mut SplatCtx) -> c_int;
    pub fn splat_frames_dropped(ctx: *const SplatCtx) -> u64;
    pub fn splat_frames_retained(ctx: *mut SplatCtx, n: *mut u64) -> c_int;
    pub fn splat_device_bytes(ctx: *const SplatCtx, peak: *mut u64) -> u64;
    pub fn splat_binning_mode(ctx: *mut SplatCtx) -> i64;
    pub fn splat_set_frame_overlap(ctx: *mut SplatCtx, n: i32) -> c_int;   // 2: frames to different images composite side by side
    pub fn splat_set_option(ctx: *mut SplatCtx, option: i32, value: f64) -> c_int;   // SPLAT_OPT_*: what the SPLAT_* environment variables set, from code
    pub fn splat_get_option(ctx: *const SplatCtx, option: i32, value: *mut f64) -> c_int;
    pub fn splat_stream(ctx: *mut SplatCtx) -> *mut c_void;               // the hipStream_t the kernels run on
    pub fn splat_set_stream(ctx: *mut SplatCtx, hip_stream: *mut c_void) -> c_int;
    pub fn splat_get_timing(ctx: *mut SplatCtx, ms: *mut f64 /* [6] */, frames: *mut u64, reset: i32) -> c_int;
    pub fn splat_get_records(ctx: *mut SplatCtx, out: *mut SplatRecord, n: u64) -> c_int;
    pub fn splat_get_tile_lists(ctx: *mut SplatCtx, tile_offsets: *mut u32, n_offsets: u64, order: *mut u32, n_order: u64) -> c_int;
    // viewer loop (src/main.rs:69-78): cleared frame, asynchronous copy-out into pinned frames
    pub fn splat_render_stream(ctx: *mut SplatCtx, cam: *const SplatCamera, argb_out: *mut u32) -> c_int;
    pub fn splat_stream_wait(ctx: *mut SplatCtx, argb_out: *const u32) -> c_int;
    pub fn splat_host_alloc(bytes: u64) -> *mut c_void;
    pub fn splat_host_free(p: *mut c_void);
    pub fn splat_host_register(p: *mut c_void, bytes: u64) -> c_int;      // pin a buffer the caller owns (e.g. Buffer2d's storage), once
    pub fn splat_host_unregister(p: *mut c_void) -> c_int;
    // device images for a host without a HIP toolchain of its own
    pub fn splat_device_alloc(ctx: *mut SplatCtx, bytes: u64) -> *mut c_void;
    pub fn splat_device_free(ctx: *mut SplatCtx, d_ptr: *mut c_void);
    pub fn splat_device_upload(ctx: *mut SplatCtx, d_dst: *mut c_void, h_src: *const c_void, bytes: u64) -> c_int;
    pub fn splat_device_download(ctx: *mut SplatCtx, h_dst: *mut c_void, d_src: *const c_void, bytes: u64) -> c_int;
    // multi-GPU, one process (B): what a multi-GPU render_to_buffer binds
    pub fn splat_multi_create(cfg: *const SplatConfig, devices: *const i32, n_devices: i32, out: *mut *mut SplatMulti) -> c_int;
    pub fn splat_multi_destroy(m: *mut SplatMulti);
    pub fn splat_multi_last_error(m: *const SplatMulti) -> *const c_char;
    pub fn splat_multi_upload_scene(m: *mut SplatMulti, n: u64, pos4: *const f32, cov3d: *const f32,
                                    opacity: *const f32, sh: *const f32) -> c_int;
    pub fn splat_multi_balance(m: *mut SplatMulti, cam: *const SplatCamera) -> c_int;
    pub fn splat_multi_set_frame_overlap(m: *mut SplatMulti, n: i32) -> c_int;
    pub fn splat_multi_get_slabs(m: *const SplatMulti, slabs_out: *mut i32) -> c_int;
    pub fn splat_multi_image(m: *mut SplatMulti) -> *mut c_void;
    pub fn splat_multi_ctx(m: *mut SplatMulti, rank: i32) -> *mut SplatCtx;
    pub fn splat_multi_render(m: *mut SplatMulti, cam: *const SplatCamera, argb: *mut u32, stats: *mut SplatStats) -> c_int;
    pub fn splat_multi_render_frame(m: *mut SplatMulti, cam: *const SplatCamera) -> c_int;
    pub fn splat_multi_sync(m: *mut SplatMulti) -> c_int;
    pub fn splat_multi_download(m: *mut SplatMulti, argb_out: *mut u32, w: i32, h: i32) -> c_int;
    // multi-GPU, one process per GPU (A)
    pub fn splat_comm_unique_id(id: *mut u8 /* [128] */) -> c_int;
    pub fn splat_comm_init_rank(ctx: *mut SplatCtx, id: *const u8, n_ranks: i32, rank: i32) -> c_int;
    pub fn splat_slab_partition(row_loads: *const u64, n_rows: i32, n_ranks: i32, row_overhead: f64,
                                slabs_out: *mut i32 /* n_ranks x {row0,row1} */) -> c_int;
    pub fn splat_comm_set_slabs(ctx: *mut SplatCtx, slabs: *const i32) -> c_int;
    pub fn splat_comm_gather(ctx: *mut SplatCtx, d_argb: *mut c_void, w: i32, h: i32, root: i32) -> c_int;
    pub fn splat_comm_loopback(ctx: *mut SplatCtx, on: i32) -> c_int;
    pub fn splat_comm_destroy(ctx: *mut SplatCtx);
}
