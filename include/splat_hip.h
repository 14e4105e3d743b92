/*
 * splat_hip.h -- C ABI of libsplat_hip.so, the MI355X (gfx950) drop-in for the
 * rasterisation hot path of thomasantony/splat.
 *
 * The reference has no FFI; its operator surface for this path is the Rust API
 *     GaussianSplatPipeline01::render_to_buffer(&self, &mut euc::Buffer<u32,2>)   src/pipelines.rs:66-86
 *     GaussianSplatPipeline02::render_to_buffer(...)                              src/pipelines.rs:260-280
 * which internally runs sort (src/gaussians.rs:297-306, 464-471), the euc vertex
 * stage (src/pipelines.rs:96-125 / 184-213 -> src/gaussians.rs:40-99, 114-161,
 * 473-522; src/pipelines.rs:17-51), euc's triangle rasteriser, fragment
 * (src/pipelines.rs:127-145) and blend (src/pipelines.rs:147-168).
 * The entry points below are what a Rust `extern "C"` block in that crate binds
 * (INTEGRATION.md shows the stub); every signature uses plain pointers and sizes.
 *
 * Conventions: all matrices column-major f32 (nalgebra storage); pixels are
 * 0xAARRGGBB u32, row-major, `w*h` of them; every function returns SPLAT_OK or
 * a negative error code and never throws/unwinds across the boundary;
 * splat_last_error() gives the message.  One splat_ctx per host thread/GPU.
 */
#ifndef SPLAT_HIP_H
#define SPLAT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPLAT_OK 0
#define SPLAT_ERR_INVALID (-1)   /* bad argument                                          */
#define SPLAT_ERR_HIP (-2)       /* HIP runtime error (no device, OOM, launch failure)    */
#define SPLAT_ERR_NO_SCENE (-3)  /* render before upload                                  */
#define SPLAT_ERR_CAPACITY (-4)  /* (Gaussian,tile) pair buffer could not be grown        */

#define SPLAT_TILE 16            /* 16x16 pixel tiles                                     */

/* Version of this header's struct layouts and entry points.  splat_abi_version() returns the one the LIBRARY was built
 * with: a binding compiled against another header (splat_stats grew by two fields between versions 4 and 5; a caller that
 * passes the shorter struct has 16 bytes written past it) compares the two before its first call -- the ctypes binding,
 * rust/src/pipelines_hip.rs and the C++ host mirror all do -- and splat_stats_size() tells the byte count it will write. */
#define SPLAT_ABI_VERSION 7
/* Added under version 7, with no change to any struct or earlier entry point: splat_decode_ply_device and
 * splat_upload_ply_device (and the splat_ply_layout they take).  A library of version 7 may predate them: a binding
 * that wants them finds them by symbol (dlsym / hasattr) and does without them where they are missing.  Likewise
 * splat_update_scene_device and splat_update_gaussians_device (and the SPLAT_FIELD_* bits they take), and
 * splat_select_device and splat_selection_indices_device (and the splat_select_query and SPLAT_SEL_* values they take), and
 * splat_read_scene_device, splat_read_gaussians_device, splat_transform_scene_device and splat_transform_gaussians_device, and
 * splat_sh_rotation_blocks, splat_rotate_sh_scene_device and splat_rotate_sh_gaussians_device, and
 * splat_select_neighbours_device, and splat_encode_ply_scene_device and splat_encode_ply_gaussians_device, and
 * splat_pick_device (and the splat_pick_query, splat_pick_result, splat_pick_layer and SPLAT_PICK_* values it takes), and
 * splat_remove_gaussians_device (and the SPLAT_REMOVE_* values it takes), and
 * splat_append_gaussians_device and splat_reorder_scene_device, and
 * splat_eval_colours_device, splat_select_colour_device (and the splat_colour_query it takes), splat_recolour_scene_device
 * and splat_recolour_gaussians_device, and
 * splat_visibility_device (and the splat_visibility_query and SPLAT_VIS_* values it takes) and splat_select_counts_device. */

/* modes: bit flags, 0 = the default */
#define SPLAT_MODE_EXACT 0       /* back-to-front, 8-bit truncation per splat as blend() does it; the exponential of
                                    fragment() is the device's (~1.5 ulp): within 1 LSB of libm's on ~1e-5 of the pixels */
#define SPLAT_MODE_CORRECTED_PROJECTION 1 /* same compositing, but cov2d = J W S W^T J^T with the perspective-shear
                                    terms of J (3DGS paper) that the reference drops (its Matrix3::new is
                                    row-major, src/gaussians.rs:141-151).  NOT parity with the reference:
                                    SURVEY section 8(f) rank 2, off by default.                                  */
#define SPLAT_MODE_LIBM_EXP 2    /* fragment()'s exp computed exactly as glibc's expf does (in double, table + cubic):
                                    the frame is then the CPU restatement's frame bit for bit.  A verification mode:
                                    ~1.5x the compositor's time.  May be combined with the flag above.               */
#define SPLAT_MODE_FAST 4        /* the compositor's early-out stops proving the frame EXACT and proves it within one
                                    count instead: the layers behind the walk's start are bracketed as in the exact
                                    mode ([lo,hi] from 0 and from 255, blend() is monotone), but the bracket counts as
                                    closed at hi - lo <= 2 and the walk continues from its MIDDLE (within 1 of the
                                    exact state; blend() never expands a difference of integer states), which half
                                    the optical depth achieves.  Every R, G, B byte is within 1 of the
                                    SPLAT_MODE_EXACT frame's (the alpha byte is the same); about a third less
                                    compositor time.  (SPLAT_FAST_WIDTH=1: closed at hi - lo <= 1, continue from lo.)  The north_star's "front-to-back ... early-out
                                    on saturated alpha", with the error bound proven instead of hoped for.        */

typedef struct splat_ctx splat_ctx;

typedef struct {
    int32_t device;        /* HIP device ordinal                                          */
    int32_t mode;          /* SPLAT_MODE_*                                                */
    /* euc conventions; splat_default_config() documents defaults  */
    int32_t y_up;          /* 1: NDC +y is row 0                                          */
    int32_t sample_half;   /* 1: sample at pixel centres                                  */
    int32_t zclip;         /* 1: cull quads with ndc.z outside [zmin,zmax]                */
    float zmin, zmax;
    uint64_t pair_capacity;/* initial (Gaussian,tile) pair capacity; 0 = auto; grows      */
} splat_config;

/* Per-frame constants = what Camera's getters return (src/camera.rs:70-93). */
typedef struct {
    float view[16];        /* Camera::get_view_matrix                                     */
    float proj[16];        /* Camera::get_project_matrix                                  */
    float w, h;            /* Camera::w, Camera::h                                        */
    float htanx, htany, focal; /* Camera::get_htanfovxy_focal                             */
    float cam_pos[3];      /* Camera::position (the field, src/pipelines.rs:99)           */
    float lowpass;         /* 0.01 for Pipeline01 (gaussians.rs:156), 0.3 for Pipeline02 (:517) */
    int32_t sh_dim;        /* 15 at both call sites (src/pipelines.rs:100,189)            */
} splat_camera;

typedef struct {
    uint64_t n_gaussians;
    uint64_t n_visible;    /* Gaussians with >= 1 covered sample in this context's slab    */
    uint64_t n_singular;   /* det(cov2d) == 0: skipped (the reference panics, pipelines.rs:22) */
    uint64_t n_pairs;      /* D = (visible Gaussian, tile) overlaps                        */
    uint64_t max_tile_len; /* longest per-tile list                                        */
    uint64_t bytes_algorithmic; /* N*148 + n_visible*48 + D*60 + w*h*4   */
    /* device time of the last frame per kernel, ms (HIP events on the context's stream)  */
    float ms_preprocess, ms_scan, ms_emit, ms_sort, ms_composite, ms_total;
    uint64_t n_fallback;   /* compositor waves whose early-out could not be proven exact and were redone in full */
    uint64_t n_sort_fallback; /* tiles re-sorted by the exact bitonic network because depth ties were out of index order */
    uint64_t n_iter_scan;  /* compositor (wave, record) iterations spent in the front-to-back scan           */
    uint64_t n_iter_blend; /* ... and in exact blending (both measured on the frame the stats belong to)     */
    uint64_t n_blocks_culled; /* 256-Gaussian blocks K1 skipped: bounds cannot reach the slab / target      */
    uint64_t flops_algorithmic; /* sum over pixels of (its tile's list length) * 25  */
    uint64_t n_near_tiles;    /* tiles whose list of more than 2048 keys was served by its selected nearest keys       */
    uint64_t n_near_fallback; /* ... of which the whole list had to be sorted after all (a walk reached the selection's far end) */
} splat_stats;

/* Projected per-Gaussian record as the kernels keep it (debug / stage parity). */
typedef struct {
    float cx, cy, hx, hy;           /* quad centre and 3-sigma half extents, pixels        */
    float conic_a, conic_b, conic_c, opacity;
    float r, g, b, depth;           /* SH colour + 0.5 (unclamped); view-space z           */
    int32_t px0, px1, py0, py1;     /* exactly covered inclusive pixel range; px0>px1 = culled */
} splat_record;

uint32_t splat_abi_version(void);    /* SPLAT_ABI_VERSION of the library */
uint64_t splat_stats_size(void);     /* sizeof(splat_stats) as the library writes it */
void splat_default_config(splat_config* cfg);
int splat_create(const splat_config* cfg, splat_ctx** out);
void splat_destroy(splat_ctx* ctx);
const char* splat_last_error(const splat_ctx* ctx);   /* ctx may be NULL: last create() error */

/* Scene upload: exactly GaussianList's buffers (src/gaussians.rs:408-416):
 * pos4 = positions.as_slice() (4n: x,y,z,1), cov3d = 3x3 column-major blocks (9n),
 * opacity (n), sh (48n, f_dc then f_rest un-transposed).  Host pointers; copied.
 * Precondition of SPLAT_MODE_LIBM_EXP only: every opacity below 1 / (255 expf(-87)) ~ 2.4e35.  That mode's
 * exponential stops falling at expf(-87) (splat_device_math.h, exp_libm), so a fragment whose exponent lies below -87
 * is rejected like the reference's only while opacity * expf(-87) < 1/255.  Any float is accepted; nothing checks it. */
int splat_upload_scene(splat_ctx* ctx, uint64_t n, const float* pos4, const float* cov3d,
                       const float* opacity, const float* sh);

/* compute_cov3d (src/gaussians.rs:101-113, 446-462) on the GPU.  scales3 (3n, already exp'd),
 * rot4 (4n, nalgebra coords order i,j,k,w, un-normalised), cov3d_out (9n).  Host pointers. */
int splat_compute_cov3d(splat_ctx* ctx, uint64_t n, const float* scales3, const float* rot4,
                        float* cov3d_out);

/* The buffers of splat_upload_scene, but in DEVICE memory of the context's GPU (same layouts: pos4 4n, cov3d 9n
 * col-major blocks, opacity n, sh 48n).  producer_stream: the hipStream_t the caller's work that wrote them was
 * enqueued on (NULL = the caller has already synchronised); the library orders itself behind it with an event.
 * Synchronous like splat_upload_scene: on return the inputs may be freed or overwritten.  Nothing of the scene
 * crosses PCIe: the Morton order, the block bounds and the packing are computed on the GPU, with the results of
 * splat_upload_scene bit for bit (every frame afterwards is the same frame). */
int splat_upload_scene_device(splat_ctx* ctx, uint64_t n, const void* d_pos4, const void* d_cov3d,
                              const void* d_opacity, const void* d_sh, void* producer_stream);
/* compute_cov3d with device in, device out (no copies); producer_stream as above.  Returns when d_cov3d_out is written. */
int splat_compute_cov3d_device(splat_ctx* ctx, uint64_t n, const void* d_scales3, const void* d_rot4,
                               void* d_cov3d_out, void* producer_stream);
/* The scene from PLY vertex rows in DEVICE memory (the INRIA layout of SURVEY.md appendix C, or any other property
 * list): what load_from_ply does between the file and the upload (src/gaussians.rs:246-283, 375-405) -- exp of the
 * scales, the sigmoid of the opacity, the quaternion reordered, the mean position subtracted, that mean from ONE
 * sequential f32 sum in index order -- on the GPU, with the host loader's results bit for bit.
 * splat_ply_layout says where in a row the float32 property feeding each destination slot lies.  Slots: */
#define SPLAT_PLY_SLOT_POS 0      /* 0-2   x y z                                   -> pos4 (w = 1)            */
#define SPLAT_PLY_SLOT_SCALE 3    /* 3-5   scale_0..2, expf                        -> scales3                 */
#define SPLAT_PLY_SLOT_OPACITY 6  /* 6     opacity, 1 / (1 + expf(-v))             -> opacity                 */
#define SPLAT_PLY_SLOT_ROT 7      /* 7-10  rot_1 rot_2 rot_3 rot_0                 -> rot4 (i, j, k, w)       */
#define SPLAT_PLY_SLOT_SH 11      /* 11-13 f_dc_0..2, 14-58 f_rest_0..44           -> sh[0..48), no transpose */
#define SPLAT_PLY_SLOTS 59
typedef struct {
    uint64_t n;                       /* vertices */
    uint32_t stride;                  /* bytes per vertex row, >= 1 */
    int32_t  offset[SPLAT_PLY_SLOTS]; /* byte offset in a row of the float32 property feeding slot k, -1 = absent */
} splat_ply_layout;
/* An absent property keeps Gaussian::new's value: 0 (a scale of 0, not exp(0); an opacity of 0), the quaternion
 * (0, 0, 0, 1).  Nothing is assumed about alignment: d_rows may be any byte address, the stride any number >= 1 (files
 * with uchar properties have strides like 251); little-endian floats are put together from the bytes they occupy.
 * SPLAT_ERR_INVALID, before any device work: a NULL context, layout or (with n > 0) pointer, stride == 0, an offset
 * below -1, offset + 4 > stride.
 * splat_decode_ply_device: into the caller's five device buffers (pos4 4n, scales3 3n, opacity n, rot4 4n, sh 48n
 * floats, 4-byte aligned), all required.  producer_stream as for splat_upload_scene_device; synchronous. */
int splat_decode_ply_device(splat_ctx* ctx, const splat_ply_layout* layout, const void* d_rows, void* d_pos4,
                            void* d_scales3, void* d_opacity, void* d_rot4, void* d_sh, void* producer_stream);
/* splat_upload_ply_device: the same chain into temporaries of the library, then cov3d -- compute_cov3d (kernel K0) when
 * compute_cov3d != 0, which is GaussianList::from_vec and the loop of src/main.rs:24-26; all zero otherwise, which is
 * Gaussian::new -- then splat_upload_scene_device.  Nothing returns to the host.  Synchronous: on return d_rows may be
 * freed and the temporaries are gone.  n == 0: as splat_upload_scene_device with n == 0. */
int splat_upload_ply_device(splat_ctx* ctx, const splat_ply_layout* layout, const void* d_rows, int32_t compute_cov3d,
                            void* producer_stream);
/* The way back: the RESIDENT scene written as PLY vertex rows into device memory of the caller -- the inverse of
 * splat_decode_ply_device, what an editor needs to keep what it did (load, select, edit, save) without a host copy of the
 * scene.  The scene holds cov3d and an opacity; a row holds three log scales, a quaternion and a logit: every Gaussian's
 * covariance is decomposed (a double-precision Jacobi iteration, S = V diag(lam) V^T with det V = +1), scale_k =
 * 0.5 ln(lam_k), (rot_1 rot_2 rot_3 rot_0) = the unit quaternion of V with rot_0 >= 0, opacity = ln(o / (1 - o)).  What
 * has no logarithm is clamped so that the loader reads back what the scene holds: lam <= 0 (a cov3d left zero, a
 * rank-deficient matrix) -> scale -104, whose expf is exactly 0; o <= 0 -> -104 (the sigmoid is exactly 0: a Gaussian
 * deleted by opacity 0 stays deleted); o >= 1 -> +104 (exactly 1); NaN stays NaN; no infinity is written for a finite
 * opacity.  The arithmetic is splat_amd/csrc/splat_ply_encode_math.h, which calls no libm: the rows are the same bits on
 * the device and in a host compile of that header.
 * WHAT A SAVE KEEPS.  Positions and all 48 sh floats keep their bits (pos4's w is no property).  Covariances and opacities
 * come back through the loader (expf, normalisation, compute_cov3d in f32) NOT bit for bit but within the error of a
 * float64 eigen-decomposition rounded to f32 the same way (profiles/ply_save_accuracy.json: max |S' - S| / ||S||_F of some
 * 10-20 units of 2^-24).  load_from_ply subtracts the mean position on every load: a reloaded scene is the saved one
 * minus its sequential-f32 mean.
 * The layout is the decoder's: offset[k] = where slot k's float goes in a row, -1 = not written; every byte of a row that
 * no present slot names (nx ny nz, padding) is written as 0.  Unlike the decoder, the encoder writes whole dwords and
 * stages every row in LDS -- it has no unstaged path: d_rows_out, stride and every present offset must be multiples of 4,
 * and stride <= 65528.  Row t is Gaussian t of the scene (layout->n == the resident n), or, indexed, Gaussian d_index[t]
 * (layout->n == k; u32 original indices in device memory, any order, duplicates allowed, as splat_read_gaussians_device
 * takes them; producer_stream: where they were written).  Exactly layout->n * stride bytes are written.
 * SPLAT_ERR_INVALID with the argument named, nothing written, and -- whatever can be judged without it -- before the
 * context is looked at: a NULL layout, a misaligned d_rows_out, stride or offset, stride == 0 or above 65528, an offset
 * below -1 or reaching beyond stride, two present offsets that overlap, a NULL d_rows_out or d_index with rows to write,
 * layout->n that is neither the resident n nor k, an index >= n.  An empty scene and k == 0 succeed and write nothing.
 * Both are synchronous and READ the scene as splat_read_scene_device does: frames in flight end first, and nothing kept
 * from frame to frame (retained lists, hints) is lost. */
int splat_encode_ply_scene_device(splat_ctx* ctx, const splat_ply_layout* layout, void* d_rows_out);
int splat_encode_ply_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const splat_ply_layout* layout,
                                      void* d_rows_out, void* producer_stream);

/* The resident scene edited IN PLACE, n fixed: a training loop that shows its Gaussians every step, an editor that moves,
 * hides or recolours a selection, a player of an animated scene.  Nothing is freed or allocated, nothing is sorted: the
 * scene keeps the order of its last upload (splat_get_scene_layout's orig_out does not change) and only the named fields'
 * values are rewritten.  A frame does not depend on that order, so the frames that follow are those of a fresh
 * splat_upload_scene of the edited arrays, byte for byte; an order gone stale costs culling and binning efficiency
 * (splat_stats.n_blocks_culled shows it), never a pixel -- upload again when it pays.  `fields`: */
#define SPLAT_FIELD_POS 1      /* pos4    4 floats per row (x y z are stored; w is not read, as in the uploads) */
#define SPLAT_FIELD_COV3D 2    /* cov3d   9 floats per row */
#define SPLAT_FIELD_OPACITY 4  /* opacity 1 float per row  */
#define SPLAT_FIELD_SH 8       /* sh      48 floats per row */
/* Both calls are synchronous like the uploads (on return the inputs may be freed; producer_stream as for
 * splat_upload_scene_device) and complete the frames in flight first: an asynchronous frame queued before the call shows
 * the scene as it was.  A buffer whose field is not named is not read and may be NULL.  The K1 block bounds are recomputed
 * from the resident values whenever POS or COV3D is named; the state kept from frame to frame (tile regions, sort launch
 * sizes, the per-tile hints, the frame policy) starts over as after an upload.  splat_device_bytes() does not change,
 * except that the first splat_update_gaussians_device on a scene makes the inverse of the order (4 bytes per Gaussian and
 * one byte per block, kept until the scene is replaced).
 * SPLAT_ERR_INVALID, before any device work: a NULL context, unknown bits in `fields`, a named field's pointer NULL with
 * n or k > 0, k > 0 with a NULL d_index, k > n; SPLAT_ERR_NO_SCENE: no resident scene; SPLAT_ERR_INVALID: n is not the
 * resident scene's.  fields == 0 or k == 0: SPLAT_OK, nothing done.
 * The multi-GPU layer (splat_multi_*) has no counterpart yet: update each rank's context (splat_multi_ctx) yourself.
 * splat_update_scene_device: the named fields of all n Gaussians from device buffers in splat_upload_scene's layouts,
 * indexed by ORIGINAL Gaussian index. */
int splat_update_scene_device(splat_ctx* ctx, uint64_t n, uint32_t fields, const void* d_pos4, const void* d_cov3d,
                              const void* d_opacity, const void* d_sh, void* producer_stream);
/* splat_update_gaussians_device: those fields of the k Gaussians d_index[0..k) (u32 original indices, distinct); the field
 * buffers are COMPACT: row t belongs to Gaussian d_index[t].  Only the blocks that hold an edited Gaussian get new bounds.
 * An index >= n: SPLAT_ERR_INVALID with nothing applied (the indices are checked on the device before anything is
 * written).  Duplicate indices are the caller's error: which row lands is unspecified per field; nothing faults. */
int splat_update_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, uint32_t fields, const void* d_pos4,
                                  const void* d_cov3d, const void* d_opacity, const void* d_sh, void* producer_stream);

/* The SELECTION such an edit works on, made on the GPU from the resident scene: one byte per Gaussian in the caller's device
 * memory (d_selection: n bytes at any byte address, ORIGINAL index order, nonzero = selected -- a torch.uint8 or torch.bool
 * tensor is one, so a caller may make or edit one itself; the library writes only 0 and 1), and from it the u32 indices
 * splat_update_gaussians_device takes.  Nothing crosses PCIe but the count.  A Gaussian passes a query when EVERY test the
 * query names passes (tests == 0: all pass), on its RESIDENT values -- those of the last upload and the edits since: */
#define SPLAT_SEL_VOLUME  1   /* position inside a box / ellipsoid given in world space   */
#define SPLAT_SEL_SCREEN  2   /* where the Gaussian lands on the target under `cam`       */
#define SPLAT_SEL_DEPTH   4   /* view-space z under `cam` (splat_record.depth) in a range */
#define SPLAT_SEL_OPACITY 8   /* resident opacity in a range                              */
#define SPLAT_SEL_OP_SET 0        /* selection = pass            */
#define SPLAT_SEL_OP_ADD 1        /* selection |= pass           */
#define SPLAT_SEL_OP_SUBTRACT 2   /* selection &= !pass          */
#define SPLAT_SEL_OP_INTERSECT 3  /* selection &= pass           */
typedef struct {
    uint32_t tests;            /* SPLAT_SEL_* bits; a Gaussian passes when EVERY named test passes; 0 = all pass */
    uint32_t volume_shape;     /* 0 = box, 1 = ellipsoid */
    float    world_to_unit[12];/* 3x4 row-major affine map, world -> the unit shape */
    uint32_t screen_rule;      /* 0 = centre, 1 = touch */
    int32_t  x0, y0, x1, y1;   /* inclusive pixel rectangle, clamped to the target by the library */
    float    depth_min, depth_max;
    float    opacity_min, opacity_max;
} splat_select_query;
/* With r the splat_record the vertex stage (K1) gives the Gaussian under `cam`, the context's conventions and its mode
 * (SPLAT_MODE_CORRECTED_PROJECTION: the corrected chain) -- bit for bit the record a frame of that camera is made of, on
 * the WHOLE target: a slab set on the context is ignored, so rank 0's context of a multi-GPU set serves as it is:
 *   VOLUME   u_k = ((m[4k] x + m[4k+1] y) + m[4k+2] z) + m[4k+3] in f32, unfused, in this order, m = world_to_unit;
 *            box: |u_k| <= 1 for k = 0, 1, 2; ellipsoid: (u0 u0 + u1 u1) + u2 u2 <= 1.  A NaN fails.
 *   SCREEN   r is visible (not singular, all finite, inside the z-clip when the convention is on, covering at least one
 *            sample of the target) and, with the rectangle clamped to [0, w-1] x [0, h-1] (empty: nothing passes),
 *            centre rule: (float)x0 <= r.cx < (float)(x1 + 1), the same in y, and -- with d_pixel_mask, a w*h u8 device
 *            image such as a painted lasso or brush -- mask[(int)r.cy * w + (int)r.cx] != 0;
 *            touch rule: the covered range [r.px0, r.px1] x [r.py0, r.py1] meets the rectangle (no pixel mask with it).
 *   DEPTH    depth_min <= r.depth <= depth_max, for every Gaussian, visible or not.  A NaN fails.
 *   OPACITY  opacity_min <= opacity <= opacity_max.
 * `op` combines the result with what d_selection holds: SET does not read it, the others read and write it (ADD and
 * SUBTRACT leave the bytes of Gaussians that do not pass as they are).  *count_out (nullable): the Gaussians selected
 * after the op.  cam may be NULL unless SCREEN or DEPTH is named; d_pixel_mask may be NULL.
 * Both calls are synchronous like the uploads (producer_stream as for splat_upload_scene_device), ordered on the context's
 * stream behind the frames in flight.  They READ the scene: the state kept from frame to frame, the inverse order and
 * splat_device_bytes() are as before (temporaries live for the call).
 * SPLAT_ERR_INVALID, before any device work: a NULL context or query, unknown bits in `tests`, an unknown op, volume_shape
 * or screen_rule, SCREEN or DEPTH named with a NULL cam (SCREEN: or a target that is no integer size in [1, 65535]), a
 * pixel mask with the touch rule, a NULL d_selection with a scene; SPLAT_ERR_NO_SCENE: no resident scene.
 * The multi-GPU layer needs no counterpart: every rank holds the whole scene and slabs are ignored, so one rank's context
 * (splat_multi_ctx) selects for all. */
int splat_select_device(splat_ctx* ctx, const splat_select_query* q, const splat_camera* cam, const void* d_pixel_mask,
                        uint32_t op, void* d_selection, uint64_t* count_out, void* producer_stream);
/* The indices of the nonzero bytes of d_selection[0..n), ascending, as u32 into d_index_out (4-byte aligned, `capacity`
 * entries): a valid d_index for splat_update_gaussians_device -- distinct and < n.  Needs no scene; d_selection may be any
 * byte mask at any byte address.  *count_out = how many are selected; when that is more than `capacity`, the first
 * `capacity` of them are written and the call still returns SPLAT_OK: compare the two.  n == 0: SPLAT_OK, count 0.
 * SPLAT_ERR_INVALID: a NULL context or count_out, n >= 2^32, a NULL d_selection with n > 0, a NULL or misaligned
 * d_index_out with n > 0 and capacity > 0. */
int splat_selection_indices_device(splat_ctx* ctx, uint64_t n, const void* d_selection, void* d_index_out,
                                   uint64_t capacity, uint64_t* count_out, void* producer_stream);
/* A selection BY NEIGHBOURHOOD: what no test on one Gaussian alone can say.  For every Gaussian i the call counts the other
 * Gaussians of a source set whose centres lie within `radius` of its own, and i passes when the count lies in
 * [count_min, count_max].  Floaters -- fewer than k neighbours within r: count_min = 0, count_max = k - 1.  Growing a
 * selection by r: d_source = d_selection, count_min = 1, count_max = 0xFFFFFFFF, op = SPLAT_SEL_OP_ADD.
 *   Distance  r2 = radius * radius, rounded to f32 once on the host.  For Gaussians i and j with RESIDENT centres p and q:
 *             dx = p.x - q.x, dy and dz alike; d2 = (dx dx + dy dy) + dz dz, each product and sum rounded to f32 once,
 *             unfused, in this order.  j is WITHIN REACH of i when d2 <= r2; a NaN fails.  The relation is symmetric bit for
 *             bit.  A Gaussian with a non-finite coordinate is within nobody's reach and nobody is within its own (d2 is inf
 *             or NaN, and r2 is finite).
 *   Count     c_i = the number of j != i (different Gaussians: coincident centres do count each other) that are in the
 *             source set and within reach of i.  The source set: the Gaussians whose byte in d_source is nonzero -- n bytes
 *             at any byte address, ORIGINAL index order, exactly like a selection; d_source == NULL: all Gaussians.  With
 *             count_max < 0xFFFFFFFF, c_i saturates at count_max + 1 (the library stops counting there).
 *   Pass, op  i passes when count_min <= c_i <= count_max.  `op` (SPLAT_SEL_OP_*) combines the result with d_selection
 *             exactly as splat_select_device does: the library writes only 0 and 1, ADD and SUBTRACT leave the bytes of
 *             Gaussians that do not pass as they are.  *count_out (nullable): the Gaussians selected after the op.
 *   Aliasing  d_source may be the very buffer d_selection is -- a selection grown in place: every source byte is read before
 *             any selection byte is written (the op is applied by a kernel of its own, behind the counts).
 *   Counts    d_counts_out (nullable): n u32, 4-byte aligned, ORIGINAL index order, receives the saturated c_i.
 *             d_selection may be NULL when d_counts_out is given: counts only, `op` is not used (an unknown one is still
 *             refused), and *count_out is the number of Gaussians that pass.  At least one of the two must be given.
 *   Work      A large radius on a large scene is O(n^2), so the work is bounded before any of it is done.  The library first
 *             counts the ORDERED pairs (target block, source block) of K1 blocks (256 consecutive slots: see
 *             splat_get_scene_layout), a block paired with itself included, whose resident bounds are within reach of each
 *             other: per axis g_a = max(max(lo_s[a] - hi_t[a], lo_t[a] - hi_s[a]), 0), and the pair counts when
 *             (g0 g0 + g1 g1) + g2 g2 <= r2, in f32, unfused, in this order.  A block with NaN bounds (no finite centre)
 *             is in no pair; the source mask plays no part.  *block_pairs_out (nullable) always receives that number.  When
 *             max_block_pairs != 0 and the number exceeds it: SPLAT_ERR_CAPACITY, nothing is written to d_selection or
 *             d_counts_out, and splat_last_error names both numbers.  0 = no limit.  The definition is exact, so a caller
 *             can restate it from splat_get_scene_layout's bounds; each pair costs up to 256 x 256 point tests.
 * The bounds only ever SKIP work: the gap above, evaluated in d2's order, is never larger than the d2 of any two centres
 * inside the boxes (f32 subtraction, multiplication and addition round monotonically), so the result is the all-pairs
 * result bit for bit -- also after edits, which recompute the bounds and leave the slot order stale.
 * It READS the scene as splat_select_device does: synchronous, ordered on the context's stream behind the frames in flight
 * (producer_stream: the stream that wrote d_source or d_selection), and the state kept from frame to frame, retained
 * lists included, survives.  splat_device_bytes() is as before; the temporaries (16 bytes, and 4 n bytes of counts when
 * d_counts_out is NULL) live for the call.
 * SPLAT_ERR_INVALID, judged before the context is looked at: radius NaN, negative or infinite, or radius * radius not finite
 * in f32; count_min > count_max; an unknown op; d_selection and d_counts_out both NULL; a misaligned d_counts_out.  Then a
 * NULL context: SPLAT_ERR_INVALID; no resident scene: SPLAT_ERR_NO_SCENE.
 * The multi-GPU layer needs no counterpart, as for splat_select_device: every rank holds the whole scene, so one rank's
 * context (splat_multi_ctx) selects for all. */
int splat_select_neighbours_device(splat_ctx* ctx, float radius, const void* d_source, uint32_t count_min, uint32_t count_max,
                                   uint32_t op, void* d_selection, void* d_counts_out, uint64_t max_block_pairs,
                                   uint64_t* block_pairs_out, uint64_t* count_out, void* producer_stream);
/* The PICK: which Gaussian is under a pixel, and what the pixel is made of -- where a click starts.  For up to
 * SPLAT_PICK_MAX_PIXELS query pixels of the WHOLE target of `cam`, under the context's conventions and its projection (as
 * splat_select_device sees them: a slab set on the context is ignored), Gaussian i is a HIT of pixel (x, y) when
 *   - its record r is visible (the SCREEN test's meaning, above) and r.px0 <= x <= r.px1, r.py0 <= y <= r.py1,
 *   - the reference's fragment() at the sample (sx, sy) = (x + off, y + off), off = 0.5 with sample_half else 0, is accepted:
 *       dx = sx - r.cx;  dy = y_up ? r.cy - sy : sy - r.cy;  power = -0.5 (A dx dx + C dy dy) - B dx dy   (f32, unfused, A B C = conic)
 *       rejected when power > 0;  alpha = min(0.99, opacity * expf(power));  rejected when alpha < 1/255,
 *   - alpha >= alpha_min, and
 *   - d_mask is NULL or d_mask[i] != 0 (one byte per Gaussian, ORIGINAL index order, exactly like a selection).
 * The exponential is glibc's expf bit for bit (the one SPLAT_MODE_LIBM_EXP renders with), WHATEVER mode the context renders
 * in: every alpha reported is the CPU oracle's.  So a frame in SPLAT_MODE_LIBM_EXP accepts exactly the fragments the pick
 * does; the default mode's exponential can differ from it in the last place and so disagree about a fragment whose alpha
 * sits on a threshold (1/255, alpha_min).
 *   Order     The hits of a pixel are ordered NEAREST FIRST -- the reverse of the order the reference draws them in (stable,
 *             ascending view-space z): descending r.depth and, among equal depths, descending original index.  Float
 *             comparison: -0.0 and +0.0 are equal.  (A NaN depth is never visible.)
 *   n_hits    how many hits the pixel has -- exact whatever max_hits is.
 *   front     the first hit: the Gaussian drawn last.  front_index (SPLAT_PICK_NONE without a hit), front_depth, front_alpha.
 *   surface   walking the hits nearest first with T_0 = 1, T_k = T_{k-1} * (1 - alpha_k) in f32 (the subtraction rounded,
 *             then the product, unfused) and coverage_k = 1 - T_k, the surface is the first hit with coverage_k >=
 *             coverage_min: surface_index, surface_depth and that coverage.  When no hit reaches coverage_min,
 *             surface_index = SPLAT_PICK_NONE, surface_depth = 0 and surface_coverage is the coverage after the last hit (0
 *             without a hit).  This is what a click should select: a faint floater in front of a wall does not win.  It is
 *             FLOAT transmittance, not the reference's blend, which truncates the pixel to 8 bits after every Gaussian.
 *   layers    with max_layers > 0: the first min(n_hits, max_layers) hits of pixel p in order, at d_layers[p * max_layers ..],
 *             each {index, depth, alpha, coverage_k}.  The rows behind them are left as they are.
 *   max_hits  bounds the list the library keeps per pixel (1 <= max_hits <= SPLAT_PICK_MAX_HITS).  A pixel with MORE hits gets
 *             flags |= SPLAT_PICK_TRUNCATED: n_hits and the front are still exact, surface_index = SPLAT_PICK_NONE,
 *             surface_depth = surface_coverage = 0 and none of its layer rows is written.  The other pixels of the call are
 *             unaffected and the call returns SPLAT_OK.  (The 1.5 M Gaussian benchmark cloud has about 2 000 hits on the pixels of
 *             its middle: profiles/pick.json.)
 * pixels_xy: n_pixels (x, y) pairs in HOST memory (they come from the mouse); duplicates are fine.  d_results (n_pixels
 * splat_pick_result) and d_layers are the caller's DEVICE memory, 4-byte aligned, so that pick -> indices -> edit stays on the
 * GPU.  Stream, event and synchronisation semantics are splat_select_device's: synchronous, ordered on the context's stream
 * behind the frames in flight (producer_stream: the stream that wrote d_mask), and it READS the scene: the state kept from
 * frame to frame, retained lists included, survives, and splat_device_bytes() is as before -- the one temporary (20 bytes per
 * pixel and 12 per pixel and hit of max_hits: 12 MB at the most) lives for the call.
 * SPLAT_ERR_INVALID, judged before the context is looked at, nothing written, splat_last_error names the argument: a NULL q or
 * cam, a target that is no integer size in [1, 65535], n_pixels > SPLAT_PICK_MAX_PIXELS, a NULL pixels_xy or d_results with
 * n_pixels > 0, a pixel outside [0, w) x [0, h), max_hits outside [1, SPLAT_PICK_MAX_HITS], max_layers > max_hits,
 * coverage_min not in (0, 1] (a NaN among it), a NaN alpha_min, max_layers > 0 with a NULL d_layers, a misaligned d_results
 * or d_layers.  Then a NULL context: SPLAT_ERR_INVALID; n_pixels == 0: SPLAT_OK, nothing done; no resident scene:
 * SPLAT_ERR_NO_SCENE.  The multi-GPU layer needs no counterpart, as for splat_select_device. */
#define SPLAT_PICK_MAX_PIXELS 256
#define SPLAT_PICK_MAX_HITS   4096
#define SPLAT_PICK_NONE       0xFFFFFFFFu
#define SPLAT_PICK_TRUNCATED  1u
typedef struct {
    float    alpha_min;        /* a hit's alpha is at least this; 0 = every accepted fragment */
    float    coverage_min;     /* the surface is the first hit whose coverage reaches this; in (0, 1] */
    uint32_t max_hits;         /* the list kept per pixel: 1 .. SPLAT_PICK_MAX_HITS */
    uint32_t max_layers;       /* layer rows per pixel in d_layers; 0 = none; <= max_hits */
} splat_pick_query;
typedef struct {
    uint32_t n_hits, flags, front_index;
    float    front_depth, front_alpha;
    uint32_t surface_index;
    float    surface_depth, surface_coverage;
} splat_pick_result;
typedef struct {
    uint32_t index;
    float    depth, alpha, coverage;
} splat_pick_layer;
int splat_pick_device(splat_ctx* ctx, const splat_pick_query* q, const splat_camera* cam, uint32_t n_pixels,
                      const int32_t* pixels_xy, const void* d_mask, void* d_results, void* d_layers, void* producer_stream);

/* VISIBILITY: what each Gaussian contributes to a view, occlusion taken into account -- for every Gaussian, on how many pixels
 * of a region of `cam`'s WHOLE target it is really SEEN, and how much.  The primitive behind "select what is seen under the
 * brush" and behind contribution-based pruning over a set of cameras.  Everything is exact: integers and f32 bit patterns.
 *   Hits      The hits of a pixel and their order are splat_pick_device's with alpha_min = 0 (above): the same record, the same
 *             rectangle test, the same fragment with glibc's expf whatever mode the context renders in, nearest first.  A
 *             Gaussian whose byte of d_mask (nullable; n bytes, ORIGINAL index order) is 0 does not exist for the query: it is
 *             neither counted nor occluding.  Conventions, projection mode and "a slab is ignored" are the pick's.
 *   Weights   Walking a pixel's hits nearest first with T_0 = 1:  w_k = T_{k-1} * alpha_k (one rounded f32 product), then
 *             T_k = T_{k-1} * (1 - alpha_k) (the subtraction rounded, then the product: the pick's chain).  Hit k is SEEN at
 *             the pixel when w_k >= weight_min.  T never increases and w_k <= T_{k-1}, so with weight_min > 0 a pixel stops
 *             as soon as T < weight_min -- exactly, nothing is lost; with weight_min == 0 the whole list is walked.
 *   Outputs   per Gaussian i, over the pixels of the region where it is seen, into the caller's DEVICE arrays of n entries,
 *             ORIGINAL index order, each nullable (not all three):
 *               d_pixels      uint32   how many pixels
 *               d_max_weight  float    the greatest w (0 if none); 4-byte aligned like d_pixels
 *               d_weight_sum  uint64   the sum of (uint32_t)(w * 16777216.0f), truncating: Q24 fixed point, so that the sum
 *                                      does not depend on the order the pixels arrive in; 8-byte aligned
 *   Region    the inclusive pixel rectangle [x0, x1] x [y0, y1], clamped to the target (empty: nothing is done), and with
 *             d_pixel_mask (nullable; w * h bytes, row-major, as the SCREEN test takes it) the pixels whose byte is nonzero.
 *   op        SPLAT_VIS_SET zeroes the given arrays first; SPLAT_VIS_ACCUMULATE adds (pixels, weight_sum) and maxes
 *             (max_weight, which must hold non-negative floats) on top of what they hold: a loop over cameras leaves the
 *             importance of every Gaussian over the view set on the device.
 * Synchronous, on the context's stream behind the frames in flight (producer_stream: the stream that wrote the masks and,
 * with ACCUMULATE, the arrays).  It READS the scene's values; it BINS the view like a two-pass frame does, into the first
 * frame slot's records and tile tables: frames rendered afterwards are byte for byte the frames they would have been, but
 * lists retained for a camera at rest and the tiles' region layouts start over (time only).  splat_device_bytes() may grow
 * by what the two-pass path keeps per Gaussian in that slot (16 bytes a Gaussian, made once) and, for a target of more
 * tiles than any before it, by the per-tile tables; the call's own key buffers (8 bytes per (Gaussian, tile) pair, and a mirror of as
 * many only where a tile's list exceeds 16384 keys) are freed.
 * SPLAT_ERR_INVALID, judged before the context is looked at, splat_last_error names the argument: a NULL q or cam, weight_min
 * NaN, negative or >= 1, an unknown op, a target that is no integer size in [1, 65535], a misaligned output, all three outputs
 * NULL.  Then a NULL context: SPLAT_ERR_INVALID; no resident scene: SPLAT_ERR_NO_SCENE.  An empty region: SPLAT_OK with
 * nothing written beyond what SET zeroes.  The multi-GPU layer needs no counterpart: every rank holds the whole scene.
 *
 * splat_select_counts_device turns such counts (or any n uint32 in device memory, 4-byte aligned) into a selection:
 * Gaussian i passes when count_min <= d_counts[i] <= count_max, combined with d_selection (n bytes) by `op`
 * (SPLAT_SEL_OP_*); *count_out (nullable) = the Gaussians selected afterwards.  It needs no scene.  SPLAT_ERR_INVALID, before
 * the context is looked at: count_min above count_max, an unknown op, n >= 2^32, with n > 0 a NULL or misaligned d_counts or
 * a NULL d_selection; then a NULL context.  n == 0: SPLAT_OK, *count_out = 0. */
#define SPLAT_VIS_SET        0u
#define SPLAT_VIS_ACCUMULATE 1u
typedef struct {
    float    weight_min;       /* a hit is seen when its weight is at least this; in [0, 1) */
    int32_t  x0, y0, x1, y1;   /* the region's rectangle, inclusive; clamped to the target */
    uint32_t op;               /* SPLAT_VIS_* */
} splat_visibility_query;
int splat_visibility_device(splat_ctx* ctx, const splat_visibility_query* q, const splat_camera* cam, const void* d_pixel_mask,
                            const void* d_mask, void* d_pixels, void* d_max_weight, void* d_weight_sum, void* producer_stream);
int splat_select_counts_device(splat_ctx* ctx, uint64_t n, const void* d_counts, uint32_t count_min, uint32_t count_max,
                               uint32_t op, void* d_selection, uint64_t* count_out, void* producer_stream);

/* Gaussians TAKEN OUT of the resident scene -- delete what is selected, or crop to it -- with the survivors compacted where
 * they lie: nothing crosses PCIe but one count, nothing is sorted (the survivors of a Morton-ordered scene are Morton-ordered),
 * and the memory of what went is given back.  `mode`: */
#define SPLAT_REMOVE_SELECTED   0u   /* the selected Gaussians go (delete) */
#define SPLAT_REMOVE_UNSELECTED 1u   /* the selected Gaussians stay (crop) */
/* d_selection: as splat_select_device writes it -- n bytes of device memory at any byte address, ORIGINAL index order,
 * nonzero = selected; n must be the resident scene's.  *n_out (required) = the survivors n'.  Survivors keep their relative
 * original order: the new index of one is its rank among the survivors in original index order, and from the call on every
 * index, row and selection byte the library takes or gives means the new numbering.  d_index_map_out (nullable; n u32,
 * 4-byte aligned): entry i = the new index of old Gaussian i, or 0xFFFFFFFF if it went -- what carries the caller's own
 * per-Gaussian arrays and other selections across the call.  Synchronous; producer_stream as for splat_update_*_device.
 *   n' == n   nothing went: SPLAT_OK, the identity map if asked for, and the call has READ the scene as a selection does --
 *             region layouts, hints, retained lists and the inverse order all survive.
 *   n' == 0   the context is as splat_upload_scene(n = 0) leaves it.
 *   else      an edit that also changes n: frames queued before it show the scene as it was (one found skipped stays pending
 *             for splat_sync), afterwards the context is what an upload of the survivors makes of it -- the state kept from
 *             frame to frame starts over, the inverse order is made again on first use -- except that the scene's order is
 *             the old one's without the slots that went (splat_get_scene_layout), not a new sort's.  The frames that follow
 *             are those of a fresh splat_upload_scene of the survivors, byte for byte.  splat_device_bytes() is what it is
 *             after uploading the survivors over the old scene; during the call the old scene and the new planes (256 B per
 *             survivor) exist side by side.  If those cannot be allocated: SPLAT_ERR_HIP, the old scene resident and
 *             unchanged; a failure after the old scene has gone leaves none, as a failed upload does.
 * SPLAT_ERR_INVALID with the argument named, before the context is looked at: a NULL n_out, an unknown mode, a misaligned
 * d_index_map_out, a NULL d_selection with n > 0; then a NULL context.  SPLAT_ERR_NO_SCENE: no resident scene;
 * SPLAT_ERR_INVALID: n is not the resident scene's.  A refused call writes nothing and changes nothing.
 * Device buffers of the old scene's size that the caller holds (its selections, an index list) do not shrink with it.  The
 * multi-GPU layer has no counterpart: call it on every rank's context (splat_multi_ctx) with the same mask. */
int splat_remove_gaussians_device(splat_ctx* ctx, uint64_t n, const void* d_selection, uint32_t mode, void* d_index_map_out,
                                  uint64_t* n_out, void* producer_stream);

/* Gaussians ADDED to the resident scene -- a paste, a duplicate, a second PLY merged into the open one -- without the scene
 * being read back, concatenated and uploaded again: the resident values are copied where they lie (256 B read and written
 * per resident Gaussian, nothing of them sorted), only the new rows are ordered and packed.
 * The four buffers are splat_upload_scene_device's: device memory, [m,4], [m,9], [m], [m,48] float32, and producer_stream as
 * there.  n must be the resident scene's; *n_out (required) = n + m.  The new Gaussians get the original indices
 * n .. n+m-1 in row order and every resident Gaussian keeps its index: no index map is needed.  Synchronous.
 *   m == 0   SPLAT_OK, *n_out = n, and the call has READ nothing: region layouts, hints, retained lists and the inverse
 *            order all survive, splat_device_bytes() has not moved.
 *   else     an edit that also changes n, as a removal is: frames queued before it show the scene as it was (one found
 *            skipped stays pending for splat_sync), afterwards the state kept from frame to frame starts over and the inverse
 *            order is made again on first use.  The scene's order (splat_get_scene_layout): slots 0 .. n-1 are untouched,
 *            slots n .. n+m-1 hold the new rows in the Morton order of the appended positions ALONE (their own finite box,
 *            ties in row order) -- not a new sort of everything.  The bounds of the blocks wholly below slot n keep their
 *            bits, the others are those of the values now in them.  The appended rows are stored with the bits an upload
 *            gives them, and the frames that follow are those of a fresh splat_upload_scene of the concatenated arrays, byte
 *            for byte, in every mode (depth ties go by original index, not by slot).  splat_device_bytes() is what it is
 *            after uploading the n + m Gaussians over the old scene; during the call the old scene and the new planes
 *            (256 B per Gaussian of n + m, and 16 B per new row for its sort) exist side by side.  If those cannot be
 *            allocated: SPLAT_ERR_HIP, the old scene resident and unchanged; a failure after the old scene has gone leaves
 *            none, as a failed upload does.
 * SPLAT_ERR_INVALID with the argument named, before the context is looked at: a NULL n_out, n + m >= 0xFFFFFFFF, with m > 0
 * a NULL field pointer; then a NULL context.  SPLAT_ERR_NO_SCENE: no resident scene (this call does not upload: an empty
 * context takes splat_upload_scene_device); SPLAT_ERR_INVALID: n is not the resident scene's.  A refused call writes
 * nothing, not even *n_out, and changes nothing.
 * Device buffers of the old scene's size that the caller holds (its selections, a read-back) do not grow with it: a
 * selection wants n + m bytes from here on.  The multi-GPU layer has no counterpart: call it on every rank's context
 * (splat_multi_ctx) with the same rows. */
int splat_append_gaussians_device(splat_ctx* ctx, uint64_t n, uint64_t m, const void* d_pos4, const void* d_cov3d,
                                  const void* d_opacity, const void* d_sh, uint64_t* n_out, void* producer_stream);

/* The resident scene PUT BACK IN ORDER: its slots as a fresh upload of its CURRENT values would order them.  The order of a
 * scene is the Morton order of its upload; splat_transform_gaussians_device and splat_update_gaussians_device move Gaussians
 * without moving their slots, a removal can shrink the box, an append orders only what it adds.  A stale order costs time
 * only -- frames do not depend on it -- but it costs: K1 culls by per-block bounds and splat_select_neighbours_device is
 * refused by the count of block pairs within reach, and a block with one member far away makes both worse.
 * The resident positions are read in original index order, sorted as an upload sorts them, and compared with the order
 * in place.  *moved_out (nullable) = the slots that hold another Gaussian in the new order than they do now.
 *   0        the call has READ the scene as a selection does: nothing is installed, everything kept from frame to frame
 *            survives, splat_device_bytes() is where it was.
 *   else     an edit, as a removal is, with n unchanged: the planes are gathered into the new order, every block's bounds
 *            are made again, the state kept from frame to frame starts over and the inverse order is made again on first
 *            use.  Afterwards splat_get_scene_layout gives the order and, bit for bit, the bounds of a fresh
 *            splat_upload_scene of the resident values; values and original indices are unchanged; the frames before and
 *            after are byte-identical to each other and to the fresh upload's, and so are records, tile lists and counts.
 *            During the call the old and the new planes exist side by side (256 B per Gaussian; 32 B per Gaussian of
 *            temporaries while the order is made, gone before the new planes are); splat_device_bytes() afterwards is what
 *            it is after uploading the same n over the old scene.  Allocation failures as for the append.
 * SPLAT_ERR_INVALID: a NULL context; SPLAT_ERR_NO_SCENE: no resident scene.  Synchronous.  An append followed by a reorder
 * leaves the context as splat_upload_scene_device of the concatenation does, in every observable respect.  The multi-GPU
 * layer has no counterpart: call it on every rank's context. */
int splat_reorder_scene_device(splat_ctx* ctx, uint64_t* moved_out);

/* The resident values GIVEN BACK, and changed WHERE THEY LIE: with these two an editor that moves, rotates or scales a
 * selection keeps no copy of the scene (after an upload from PLY rows it never had one), and select -> indices -> transform,
 * or -> read -> anything -> update, stays on the GPU.  The scene holds the floats of its uploads and edits losslessly, so a
 * read returns them bit for bit.
 * splat_read_scene_device is the inverse of splat_update_scene_device: the named fields (SPLAT_FIELD_* bits) of all n
 * Gaussians into the caller's device buffers, in the updates' layouts, rows in ORIGINAL index order.  pos4 gets x y z and
 * w = 1.0f (the scene does not store w; the uploads never read it).  A buffer whose field is not named is left untouched
 * and may be NULL.
 * splat_read_gaussians_device is the inverse of splat_update_gaussians_device: COMPACT rows, row t = Gaussian d_index[t]
 * (u32 original indices; producer_stream as for splat_upload_scene_device: the stream that wrote them).  Duplicate indices
 * are fine: each output row is written on its own.  An index >= n: SPLAT_ERR_INVALID and nothing is written (the indices
 * are checked on the device first).
 * Both READ the scene as splat_select_device does: synchronous, ordered on the context's stream behind the frames in
 * flight, and the state kept from frame to frame (tile regions, hints, the frame policy, retained lists) survives.
 * splat_device_bytes() is as before, except that the first indexed read of a scene makes the inverse of the order as the
 * first splat_update_gaussians_device does (4 bytes per Gaussian and one byte per block, kept until the scene is replaced),
 * unless an indexed edit has made it already.
 * SPLAT_ERR_INVALID, before any device work, as for the updates: a NULL context, unknown bits in `fields`, a named field's
 * pointer NULL with n or k > 0, k > 0 with a NULL d_index, k > n (kept for symmetry: the rows are meant to be usable as an
 * update); SPLAT_ERR_NO_SCENE: no resident scene; SPLAT_ERR_INVALID: n is not the resident scene's.  fields == 0 or
 * k == 0: SPLAT_OK, nothing done. */
int splat_read_scene_device(splat_ctx* ctx, uint64_t n, uint32_t fields, void* d_pos4, void* d_cov3d, void* d_opacity,
                            void* d_sh);
int splat_read_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, uint32_t fields, void* d_pos4,
                                void* d_cov3d, void* d_opacity, void* d_sh, void* producer_stream);
/* An affine map applied to the positions and 3D covariances of the whole scene, or of the k Gaussians d_index[0..k), in
 * place.  m: 3x4 row-major in HOST memory, world -> world, the layout of splat_select_query.world_to_unit.  With
 * A(r,k) = m[4r+k] and S(r,c) = cov[3c+r] (the blocks are column-major), every product and every sum rounded to f32 once,
 * unfused, in exactly this order:
 *   p'_r    = ((A(r,0) x + A(r,1) y) + A(r,2) z) + m[4r+3]
 *   T(r,c)  =  (A(r,0) S(0,c) + A(r,1) S(1,c)) + A(r,2) S(2,c)
 *   S'(r,c) =  (T(r,0) A(c,0) + T(r,1) A(c,1)) + T(r,2) A(c,2)        all nine, each on its own
 * which is S' = A S A^T.  Nothing is symmetrised; with the identity the values come back equal (a -0 may become +0).  Any
 * float in m is accepted; nothing checks it.  Opacity and sh keep their bits.  sh is NOT rotated: view-dependent colour
 * keeps its world-space lobes -- a caller that wants it turned reads sh, rotates it and updates it.
 * A transform is an EDIT and behaves as splat_update_* does: synchronous, the frames in flight complete first and show the
 * scene as it was, the K1 block bounds are recomputed from the resident values (of all blocks, or of those that hold a
 * mapped Gaussian), the state kept from frame to frame starts over; the frames that follow are those of a fresh
 * splat_upload_scene of the mapped arrays, byte for byte.  The indexed form checks the indices on the device before anything
 * is written (an index >= n: SPLAT_ERR_INVALID, nothing applied) and makes the inverse order like the other indexed calls.
 * Duplicate indices are the caller's error: such a Gaussian may be mapped once or twice; nothing faults.
 * SPLAT_ERR_INVALID, before any device work: a NULL context or m, k > 0 with a NULL d_index, k > n; SPLAT_ERR_NO_SCENE: no
 * resident scene.  k == 0: SPLAT_OK, nothing done.
 * The multi-GPU layer (splat_multi_*) has no counterpart, as for the updates: read from one rank's context, transform each
 * rank's (splat_multi_ctx). */
int splat_transform_scene_device(splat_ctx* ctx, const float m[12]);
int splat_transform_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const float m[12],
                                     void* producer_stream);

/* View-dependent colour TURNED WITH THE SCENE: what the transforms leave undone.  r: 3x3 row-major in HOST memory,
 * R(i,k) = r[3i+k], world -> world -- the layout of the linear part of the transform's m.  The colour of a Gaussian is
 * eval_sh(sh, dir): per channel 16 coefficients sh[3k + ch] in four bands, k = 0 | 1..3 | 4..8 | 9..15.  For an orthogonal R
 * the rotated coefficients c' satisfy eval_sh(c', R d) == eval_sh(c, d) for every unit d: band 0 keeps its bits, band l is
 * multiplied by a (2l+1) x (2l+1) block D_l(R),
 *   c'_m = (((D(m,0) c_0 + D(m,1) c_1) + D(m,2) c_2) + ...)
 * summed left to right, every product and every sum rounded to f32 once, unfused; every input of a band is read before any
 * of its outputs is written.  Nothing in sh is checked: with a non-finite coefficient 0 * inf is NaN, so one inf or NaN
 * makes its whole band of that channel NaN, also under the identity.
 * splat_sh_rotation_blocks gives the f32 blocks, row-major (d_l[(2l+1) m + k] = D_l(m,k)): host only, no context, no GPU.
 * They are derived in double from eval_sh's own polynomials and constants (this basis has its own signs and order): the
 * least-squares solution of B_l D_l = B_l^R over 32 fixed directions on a Fibonacci spiral (B_l: the band's functions at
 * d_i, B_l^R: at R^T d_i), every entry snapped to the nearest multiple of 2^-40 and then rounded to f32.  The snap (at most
 * 4.6e-13) makes the blocks of the identity, of axis-aligned quarter turns and of axis mirrors exact signed permutations:
 * the identity returns the values (a -0 may become +0), four quarter turns return the bits of every non-zero coefficient.
 * r must be orthogonal; the library checks it in double on the f32 entries: every entry finite and max |R R^T - I| <= 1e-4
 * (rotations made in f32 sit near 1e-7, a 1 % scale at 2e-2).  Otherwise SPLAT_ERR_INVALID and nothing is applied or
 * written.  Reflections (det = -1) are accepted.
 * The two device calls are EDITS and behave exactly as splat_update_* with SPLAT_FIELD_SH alone does: synchronous, the
 * frames in flight complete first and show the scene as it was, the state kept from frame to frame starts over; positions
 * and covariances stay, so the order and the K1 block bounds stay; the frames that follow are those of a fresh
 * splat_upload_scene of the rotated arrays, byte for byte.  The indexed form checks the indices on the device before
 * anything is written (an index >= n: SPLAT_ERR_INVALID, nothing applied) and makes the inverse order like the other
 * indexed calls.  Duplicate indices are the caller's error: such a Gaussian may be turned once or twice; nothing faults.
 * SPLAT_ERR_INVALID, before any device work: a NULL context or r (or d1, d2, d3), an r that is refused, k > 0 with a NULL
 * d_index, k > n; SPLAT_ERR_NO_SCENE: no resident scene.  k == 0: SPLAT_OK, nothing done.
 * The multi-GPU layer (splat_multi_*) has no counterpart, as for the updates: rotate each rank's (splat_multi_ctx). */
int splat_sh_rotation_blocks(const float r[9], float d1[9], float d2[25], float d3[49]);
int splat_rotate_sh_scene_device(splat_ctx* ctx, const float r[9]);
int splat_rotate_sh_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const float r[9],
                                     void* producer_stream);

/* COLOUR: the colour a Gaussian is drawn with under a camera, a selection by that colour (the "magic wand" that follows a
 * pick), and a 3x4 map of the colour applied where it is kept -- in the sh coefficients -- without the rows leaving the GPU.
 * With d = (p - cam_pos) / |p - cam_pos| (|v| = sqrtf((vx vx + vy vy) + vz vz), a division per component), the colour is
 *   rgb = eval_sh(sh, sh_dim, d) + 0.5
 * exactly as the vertex stage (K1) computes it for the records of a frame: band 0 always, band 1 with sh_dim > 3, band 2
 * with > 12, band 3 with > 27; the same f32 operations in the same order, so splat_record.r/g/b bit for bit -- for EVERY
 * Gaussian, visible or not, and unclamped.  A frame replaces a non-finite colour by +-FLT_MAX before it blends; these calls
 * do not: a NaN stays a NaN (a Gaussian AT the camera position has a NaN colour from band 1 on).  Of `cam` only cam_pos and
 * sh_dim are read; a slab set on the context is ignored.
 * splat_eval_colours_device: three f32 a row into d_rgb_out (device memory, 4-byte aligned).  d_index == NULL: all n
 * Gaussians in ORIGINAL index order, and k must be n.  Otherwise row t is the colour of Gaussian d_index[t] (u32 original
 * indices, in any order, duplicates allowed), k <= n rows.
 * splat_select_colour_device: the colour judged by a query in colour space, with the VOLUME test's semantics of
 * splat_select_query: with clamp != 0 each channel first becomes v < 0 ? 0 : (v > 1 ? 1 : v) (a NaN stays a NaN), then
 *   u_k = ((m[4k] r + m[4k+1] g) + m[4k+2] b) + m[4k+3] in f32, unfused, in this order, m = colour_to_unit;
 *   box: |u_k| <= 1 for k = 0, 1, 2; ellipsoid: (u0 u0 + u1 u1) + u2 u2 <= 1.  A NaN fails.
 * One map covers a ball around a picked colour (diag(1/tol) | -rgb/tol), per-channel ranges (a box) and a luminance band
 * (one row of luma weights, two zero rows).  `op`, d_selection and *count_out are splat_select_device's: the library writes
 * only 0 and 1, SET does not read the selection, ADD and SUBTRACT leave the bytes of Gaussians that do not pass as they are.
 * Both READ the scene as splat_select_device does: synchronous (producer_stream as for splat_upload_scene_device), ordered on
 * the context's stream behind the frames in flight; the state kept from frame to frame and splat_device_bytes() are as
 * before (the indexed form makes the inverse order like the other indexed calls). */
typedef struct {
    float    colour_to_unit[12];/* 3x4 row-major affine map, colour -> the unit shape */
    uint32_t shape;             /* 0 = box, 1 = ellipsoid */
    uint32_t clamp;             /* nonzero: the colour is clamped to [0, 1] per channel before the map */
} splat_colour_query;
/* splat_recolour_*: m = 3x4 row-major in HOST memory, rgb' = A rgb + t with A(i,k) = m[4i+k], t_i = m[4i+3].  The colour is
 * linear in the coefficients, so for each of the 16 coefficients k, with (r, g, b) = sh[3k .. 3k+3) read before any is
 * written,
 *   sh'[3k+i] = (A(i,0) r + A(i,1) g) + A(i,2) b        in f32, unfused, in this order,
 * and for k == 0 only that + o_i, with o_i = (t_i + 0.5 ((A(i,0) + A(i,1)) + A(i,2)) - 0.5) / C0 evaluated in double from the
 * f32 entries (C0 = 0.28209479177387814f widened) and rounded to f32 once.  In exact arithmetic eval_sh(sh', d) + 0.5 =
 * A (eval_sh(sh, d) + 0.5) + t for every direction and every sh_dim, band 0 alone included.  Nothing in sh is checked: with a
 * non-finite coefficient 0 * inf is NaN, so one inf or NaN makes all three channels of its coefficient NaN.
 * The two calls are EDITS of sh alone and behave exactly as splat_rotate_sh_*: synchronous, the frames in flight complete
 * first and show the scene as it was, the state kept from frame to frame starts over; positions and covariances stay, so
 * the order and the K1 block bounds stay; the frames that follow are those of a fresh splat_upload_scene of the recoloured
 * arrays, byte for byte.  The indexed form takes distinct indices (a Gaussian named twice may be mapped once or twice;
 * nothing faults).
 * The arguments are judged before the context is looked at, and splat_last_error names the argument.  SPLAT_ERR_INVALID: a
 * NULL q, cam or m; an unknown shape or op; a non-finite entry of m or a non-finite o; a NULL or misaligned d_rgb_out with
 * k > 0; a NULL d_selection; then a NULL context; SPLAT_ERR_NO_SCENE: no resident scene; SPLAT_ERR_INVALID: k > n, k != n
 * with a NULL d_index, and -- checked on the device before anything is written or applied -- an index >= n.  k == 0:
 * SPLAT_OK, nothing done.
 * The multi-GPU layer (splat_multi_*) has no counterpart, as for the updates: evaluate and select on one rank's context
 * (every rank holds the whole scene), recolour each rank's (splat_multi_ctx). */
int splat_eval_colours_device(splat_ctx* ctx, const splat_camera* cam, uint64_t k, const void* d_index, void* d_rgb_out,
                              void* producer_stream);
int splat_select_colour_device(splat_ctx* ctx, const splat_colour_query* q, const splat_camera* cam, uint32_t op,
                               void* d_selection, uint64_t* count_out, void* producer_stream);
int splat_recolour_scene_device(splat_ctx* ctx, const float m[12]);
int splat_recolour_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const float m[12],
                                    void* producer_stream);

/* Debug / stage parity: the stored scene order and K1 block bounds of the current scene.
 * orig_out: n u32 (slot j holds original Gaussian orig[j]); bounds_out: ceil(n/256) x 8 f32
 * (lo[3], hi[3], fmax, pad), either may be NULL.  n and n_blocks must be the scene's. */
int splat_get_scene_layout(splat_ctx* ctx, uint32_t* orig_out, uint64_t n, float* bounds_out, uint64_t n_blocks);

/* Restrict rendering to tile rows [tile_row0, tile_row1) (multi-GPU slabs); (0,-1) = all. */
int splat_set_slab(splat_ctx* ctx, int32_t tile_row0, int32_t tile_row1);

/* Load estimate for balancing slabs: (Gaussian,tile) pair count of every tile row of the FULL
 * frame for this camera (the slab setting is ignored and left unchanged).  Runs only the
 * preprocess + scan kernels.  n_rows must be ceil(h / SPLAT_TILE). */
int splat_tile_row_loads(splat_ctx* ctx, const splat_camera* cam, uint64_t* row_pairs, int32_t n_rows);

/* Viewer-loop variant (src/main.rs:69-78: clear, render, present): the frame is rendered onto a
 * CLEARED device image -- what the loop's `color.clear(0)` + `render_to_buffer` amount to -- and
 * copied to `argb_out` (host, w*h u32) asynchronously; the call returns once the work is queued.
 * Frames rotate through four device images, so up to four may be in flight: frames N+1.. render while frame N
 * crosses PCIe (two in flight is a double-buffered window; three or more keep the device's frame pipeline full).
 * `argb_out` is complete after splat_stream_wait(ctx, argb_out) (or splat_sync); give each frame
 * in flight its own buffer, ideally pinned (splat_host_alloc) -- a pageable one works but the
 * copy then blocks the calling thread.  A streamed frame that outgrew its storage on the device (tile
 * bucket, pair buffer, sort launch sizes: all sized from earlier frames) is detected by the wait, which
 * grows the storage and renders that frame again into `argb_out` before it returns: a viewer loop never
 * sees the miss (splat_frames_dropped() counts them).  On a context restricted to a slab only the slab's rows are
 * rendered; the other rows of `argb_out` read as zeros. */
int splat_render_stream(splat_ctx* ctx, const splat_camera* cam, uint32_t* argb_out);
int splat_stream_wait(splat_ctx* ctx, const uint32_t* argb_out);
void* splat_host_alloc(uint64_t bytes);      /* page-locked host memory (hipHostMalloc); NULL on failure */
void splat_host_free(void* p);
/* Page-lock a host image the CALLER owns (hipHostRegister) -- the reference's `color` buffer lives as long as the window
 * (src/main.rs:62), so it is pinned once: splat_render's copies of a pageable image go through the driver's staging
 * buffers at a fraction of the PCIe rate (C3, synchronous host in/out frame: 850 -> 990 frames/s).  Unregister before the
 * memory is freed.  SPLAT_ERR_HIP when the driver refuses (memory it cannot map). */
int splat_host_register(void* p, uint64_t bytes);
int splat_host_unregister(void* p);

/* Device images for callers without a HIP toolchain of their own (a Rust/C host using
 * splat_render_device): plain allocations on the context's GPU, and copies ordered on the context's
 * stream (the copy functions return when the data has arrived). */
void* splat_device_alloc(splat_ctx* ctx, uint64_t bytes);          /* NULL on failure (splat_last_error) */
void splat_device_free(splat_ctx* ctx, void* d_ptr);
int splat_device_upload(splat_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int splat_device_download(splat_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);

/* render_to_buffer: blends the scene onto `argb` (in/out, host, w*h u32).  stats may be NULL. */
int splat_render(splat_ctx* ctx, const splat_camera* cam, uint32_t* argb, splat_stats* stats);

/* The viewer loop's frame, host-visible: `color.clear(0); pipeline.render_to_buffer(&mut color)` (src/main.rs:73-74) as ONE
 * synchronous call.  The clear is fused into the compositor and the pixels cross PCIe once, device -> host -- splat_render
 * (in/out blending, the literal render_to_buffer) ships the caller's zeros up first: 8.3 MB each way at 1080p.  `argb_out`
 * (w*h u32) is WRITTEN, never read.  A page-locked `argb_out` (splat_host_alloc, or the caller's long-lived buffer after
 * splat_host_register: the reference's `color`, src/main.rs:62) that the device can address is written by the compositor
 * itself while the frame is being composited (zero copy, SPLAT_OPT_HOST_ZERO_COPY); any other one is filled by a copy
 * behind the compositor.  With a slab set only the slab's rows of `argb_out` are written.  stats may be NULL (and should be
 * in a loop: a statistics frame reads counters back). */
int splat_render_frame(splat_ctx* ctx, const splat_camera* cam, uint32_t* argb_out, splat_stats* stats);

/* Same with a device-resident image (in/out, w*h u32 in HBM).  Work is enqueued on the
 * context's stream; with sync != 0 (or stats != NULL) the call waits for completion. */
int splat_render_device(splat_ctx* ctx, const splat_camera* cam, void* d_argb, int32_t sync,
                        splat_stats* stats);
/* Wait for everything enqueued.  SPLAT_ERR_CAPACITY: an asynchronous frame (splat_render_device with
 * sync == 0) was skipped on the device because it outgrew its storage -- its image was left untouched and
 * the storage has been grown: render it again.  Reported once.  A synchronous render redoes its OWN frame
 * internally and never returns this code for a frame that composited. */
int splat_sync(splat_ctx* ctx);
/* The viewer loop's frame on a device image: `color.clear(0); render_to_buffer(&mut color)` (src/main.rs:73-74) in one
 * call -- the clear is fused into the compositor (old pixels are not read; tiles nothing covers are zeroed), so the
 * frame costs no separate pass over the image.  Same result, byte for byte, as a memset followed by
 * splat_render_device.  With a slab set, only the slab's rows are cleared and rendered. */
int splat_render_frame_device(splat_ctx* ctx, const splat_camera* cam, void* d_argb, int32_t sync, splat_stats* stats);
uint64_t splat_frames_dropped(const splat_ctx* ctx);  /* frames skipped on the device since splat_create (redone or reported) */
/* *n = frames since splat_create that were composited from RETAINED LISTS (SPLAT_OPT_RETAIN_LISTS): the lists an earlier frame
 * of the same camera left in order in memory -- no preprocess, scan, selection or sort of their own. */
int splat_frames_retained(splat_ctx* ctx, uint64_t* n);
/* Device memory this context holds right now (scene planes, per-frame buffers of its frame slots, key buffers, images it
 * allocated); *peak (nullable) = the most it has held since splat_create. */
uint64_t splat_device_bytes(const splat_ctx* ctx, uint64_t* peak);
/* Frame overlap for SWAP CHAINS (default 1; SPLAT_FRAME_OVERLAP=2 sets it at splat_create).  The reference's loop clears and
 * renders ONE buffer per frame (src/main.rs:71-75), and so does every entry point above: the compositors of consecutive
 * frames run one after the other, in call order, on the context's stream.  A frame that is bound by the latency of its
 * densest tile's lone wavefront -- a small scene, a tile-row slab of a multi-GPU frame -- then leaves most of the chip idle.
 * With n = 2 an ASYNCHRONOUS frame (sync == 0, stats == NULL) to an image that no frame in flight touches composites on
 * a second internal stream, beside the previous frame's compositor: alternate two device images and two frames share
 * the chip (C2: 5.7 k -> 7.9 k frames/s, an eighth-of-a-frame slab of C3: 0.13 -> 0.08 ms per frame).  Frames to the SAME image
 * keep their call order (stream order on one lane: in/out blending and clear+render behave as before), synchronous
 * frames order themselves behind everything in flight, splat_comm_gather follows the frame rendered last.  What changes:
 * an overlapped frame is no longer ordered against work the CALLER enqueues on splat_stream() -- use splat_sync (or a
 * synchronous frame) before touching a target image from a stream of your own.  splat_render_stream's frames are not
 * overlapped (the second compositor stream is the one their copies to the host travel on: a stream more would share a
 * hardware queue with a busy one). */
int splat_set_frame_overlap(splat_ctx* ctx, int32_t n);
/* Tuning options of a context, for hosts that cannot (or should not) reach them through the environment -- a Rust or C
 * application sets them after splat_create.  None of them changes a pixel of an exact-mode frame: they choose between equivalent schedules
 * and storage sizes (SPLAT_MODE_FAST frames stay within 1 of the exact frame per colour byte whatever
 * SPLAT_OPT_EARLY_OUT_EPS / SPLAT_OPT_FAST_CLOSE_WIDTH say, but which of those frames it is depends on them).  The SPLAT_* environment variable of the same purpose, when set, is read at splat_create and
 * PINS the option: a later splat_set_option on it leaves the operator's value in force and returns SPLAT_OK
 * (splat_get_option tells what is in force).  splat_set_option waits for the frames in flight; options that size
 * storage (pipeline depth, key buffer bytes, one-pass binning) take effect with the next frame, which re-allocates.
 * SPLAT_ERR_INVALID: unknown option or value out of range (the range is in the comment of each). */
#define SPLAT_OPT_PIPELINE_DEPTH 1       /* frames in flight on the device, 1..6 (default 6; SPLAT_PIPELINE): 1 = one stream, no
                                            cross-frame overlap; 2 = binning + sort of frame N+1 under the compositor of frame N;
                                            6 = four frame slots, two binning chains in flight                                   */
#define SPLAT_OPT_FUSED_SORT_MAX 2       /* lists up to this many keys are sorted by their tile's compositor workgroup, 0..2048
                                            (default 2048; SPLAT_FUSED_SORT); 0 = every list goes through the sort launches      */
#define SPLAT_OPT_REGION_SPARE 3         /* one-pass binning: how far a tile's key region may grow into the buffer's spare room,
                                            >= 1 (default 4; SPLAT_REGION_SPARE): larger tolerates larger camera jumps           */
#define SPLAT_OPT_EARLY_OUT_EPS 4        /* transmittance below which the compositor's near-to-far scan stops, 0..1 (default
                                            1e-6, 2e-3 in SPLAT_MODE_FAST; SPLAT_EARLY_EPS); 0 switches the early-out off       */
#define SPLAT_OPT_EARLY_OUT_MIN_LIST 5   /* shortest tile list that gets the early-out scan, >= 0 (default 768, 384 in
                                            SPLAT_MODE_FAST; SPLAT_EARLY_MIN)                                                    */
#define SPLAT_OPT_EARLY_OUT_SCAN_EIGHTHS 6 /* the scan gives up after this many eighths of the list, 1..8 (default 4;
                                            SPLAT_EARLY_SCAN8)                                                                   */
#define SPLAT_OPT_SORT_IN_COMPOSITOR 7   /* who sorts lists of more than 2048 keys: 0 = sort launches, 1 = the tile's compositor
                                            workgroup, -1 = chosen per frame from the previous frame (default; SPLAT_SORT_IN_COMP) */
#define SPLAT_OPT_PAIR_WALK 8            /* the exact walk takes two records per step with packed math: 0 / 1, -1 = per frame
                                            from the previous frame's statistics (default; SPLAT_PAIR_BLEND)                     */
#define SPLAT_OPT_TIMING_EVERY 9         /* per-kernel timing events ride on every n-th asynchronous frame, >= 1 (default 8;
                                            SPLAT_TIMING_EVERY)                                                                  */
#define SPLAT_OPT_BLOCK_CULLING 10       /* K1 skips 256-Gaussian blocks whose bounds cannot reach the slab / target: 0 / 1
                                            (default 1; SPLAT_CULL)                                                              */
#define SPLAT_OPT_ONE_PASS_BINNING 11    /* per-tile key regions filled by K1 itself (no count / emit passes): 0 / 1 (default 1;
                                            SPLAT_BUCKETS)                                                                       */
#define SPLAT_OPT_KEY_BUFFER_BYTES 12    /* ceiling on the key buffers of all frame slots together for one-pass binning, bytes
                                            (default 128 GiB; SPLAT_BUCKET_BYTES): beyond it the two-pass path is used          */
#define SPLAT_OPT_FAST_CLOSE_WIDTH 13    /* SPLAT_MODE_FAST: the bracket counts as closed at hi - lo <= 1 or 2 (default 2;
                                            SPLAT_FAST_WIDTH)                                                                    */
#define SPLAT_OPT_PRIORITY_LIST_LEN 14   /* compositor waves of lists at least this long (x2, x4) run at raised priority, >= 1
                                            (default: off; SPLAT_PRIO_LEN)                                                       */
#define SPLAT_OPT_FRAME_OVERLAP 15       /* = splat_set_frame_overlap: 1 / 2 (default 1; SPLAT_FRAME_OVERLAP)                     */
#define SPLAT_OPT_NEAR_SELECT_KEYS 16    /* near selection: of a tile list of more than 2048 keys only the nearest <= this many are
                                            selected (by depth, no sort) and put in order -- the exact early-out never looks
                                            farther on all but a few tiles, which sort their whole list after all (stats:
                                            n_near_tiles, n_near_fallback); 64..2048, 0 = off: every long list is sorted in full
                                            (default 2048; SPLAT_NEAR_KEYS)                                                      */
#define SPLAT_OPT_OVERFLOW_REDO 17       /* a frame whose camera differs from the one its tile regions were sized for carries a
                                            second binning behind its scan -- launches that leave at once unless a list outgrew its
                                            region -- so that such a frame is binned again ON THE DEVICE instead of being skipped and
                                            reported (SPLAT_ERR_CAPACITY at the next splat_sync).  0 = off; 1 = adaptive (default):
                                            only while a list has outgrown its region within the last 256 frames -- a scene that
                                            never does pays nothing; the frame of a camera JUMP carries it too; the first frame of a
                                            smooth path that outgrows a region after a quiet stretch is skipped and reported as
                                            before and arms the redo; 2 = on every frame of a moving camera (five
                                            near-empty launches per frame on the binning stream).  SPLAT_OVERFLOW_REDO           */
#define SPLAT_OPT_START_HINTS 18         /* where a compositor wave's exact walk starts is normally found by a scan of its tile's list
                                            from the near end (the early-out).  With a camera at rest the lists are the previous
                                            frame's lists: the walk starts where that frame's did (one word per wave, kept from
                                            frame to frame) and the scan is skipped; with a camera that moved by less than about
                                            half a degree since the last frame, where it did plus an eighth, three frames of four.
                                            A start that turns out too shallow is retried deeper, as after any scan: exactness
                                            never rests on the hint.  0 = scan every frame; 1 = camera at rest only; 2 = at rest
                                            and in slow motion (default 2; SPLAT_START_HINTS)                                    */
#define SPLAT_OPT_HOST_ZERO_COPY 19      /* splat_render_frame into a page-locked image the device can address: 1 = the compositor
                                            stores its pixels straight into host memory (the image crosses PCIe under the frame),
                                            0 = device image + a copy behind the frame (default 1; SPLAT_HOST_ZERO_COPY)           */
#define SPLAT_OPT_KEYS_PER_GAUSSIAN 20   /* one-pass binning: entries of a frame slot's key buffer per Gaussian of the scene, 4..256,
                                            0 = by the scene's size (default; SPLAT_KEYS_PER_GAUSSIAN).  What the tiles' regions do
                                            not ask for is their room to grow under a moving camera (SPLAT_OPT_REGION_SPARE)       */
#define SPLAT_OPT_COUNT_FIRST 21         /* one-pass binning: which frames count their pairs per tile first (K1's count flavour: geometry
                                            only, a third of a K1) and bin into regions that fit exactly their own camera, instead of
                                            into regions sized from the frame two back: 0 = only a frame slot without regions (first
                                            frames, a new scene / target / slab); 1 (default) = also the next 64 frames of a moving
                                            camera once three in four of the recent frames binned into another camera's regions
                                            outgrew them (were binned twice by the overflow redo, or skipped) -- under every
                                            SPLAT_OPT_OVERFLOW_REDO setting; the frame of a camera jump does NOT count first (it
                                            carries the redo launches instead); 2 = also every frame whose camera moved by more than
                                            half a degree.  The rule is include/splat_policy.h (SPLAT_COUNT_FIRST)                    */
#define SPLAT_OPT_LARGE_SPLAT_TILES 22   /* one-pass binning: a splat of more tiles than this -- and every splat wider or taller than the
                                            projection kernel's 32 x 32-tile window -- is not expanded pair by pair with global atomics by
                                            its K1 block; it goes to the frame's large list, which a second kernel bins tile by tile
                                            (a camera inside the scene: K1 1.1 -> 0.18 ms on 1.5 M Gaussians).  0 = the window alone
                                            decides, -1 = no list (default 128; SPLAT_LARGE_TILES)                                  */
#define SPLAT_OPT_LARGE_LIST_MIN 23      /* ... and frames keep such a list only while the last frame the host has heard from had at
                                            least this many large splats (half of it to let go again; always when nothing is known
                                            or behind a camera jump): the list's kernel is one more launch on a small frame's chain.
                                            0 = always, -1 = never (default 256; SPLAT_LARGE_LIST_MIN; include/splat_policy.h)        */
#define SPLAT_OPT_START_REFINE 24       /* with a camera at rest (SPLAT_OPT_START_HINTS 1 or 2) the compositor's waves refine where
                                            their exact walks start: half of the tiles a frame try a shallower start than the one
                                            that closed last, keep it where the bracket closes and walk again from the old one where it
                                            does not (those waves are not counted as n_fallback).  Exactness never rests on it.  Exact modes only (not with
                                            SPLAT_MODE_FAST, whose frame depends on where a walk starts).
                                            1 = on (default), 0 = off (SPLAT_START_REFINE)                                         */
#define SPLAT_OPT_RETAIN_LISTS 25        /* a camera at rest composites from the lists an earlier frame left in order: once the camera
                                            the calls receive has been the same, byte for byte, for three frames, one frame stores its
                                            sorted lists back to memory (64 MB on C3, once) and the frames behind it launch the compositor
                                            alone -- until the camera, the scene (upload, edit), the slab, the target, an option or the
                                            storage changes.  Same pixels.  Not with a frame overlap of 2, not with two-pass binning.
                                            1 = on (default), 0 = off (SPLAT_RETAIN; include/splat_retain.h)                        */
int splat_set_option(splat_ctx* ctx, int32_t option, double value);
int splat_get_option(const splat_ctx* ctx, int32_t option, double* value);
void* splat_stream(splat_ctx* ctx);                   /* the hipStream_t the kernels run on */
/* Run on a caller-owned hipStream_t (e.g. the stream a device image / RCCL gather lives on). */
int splat_set_stream(splat_ctx* ctx, void* hip_stream);
/* Accumulated per-kernel device time since the last reset, from HIP events recorded on the
 * kernels' own streams around the launches: ms[0..5] = preprocess, scan, emit, sort, composite,
 * status read-back; *frames = frames that carried events.  Event records cost queue bubbles, so
 * only every SPLAT_TIMING_EVERY-th frame (default 8) of an asynchronous run carries them, plus every
 * frame rendered with a stats pointer; averages = ms[k] / *frames.  Waits for outstanding frames.
 * With retained lists (SPLAT_OPT_RETAIN_LISTS): a retained frame that carries events adds to ms[4] and ms[5] only and counts in
 * *frames -- it has no preprocess, scan, emit or sort -- so over a camera at rest ms[0..3] / *frames tend to 0.  The frame that
 * stores the lists (one per rest) always carries the events, beyond the sampling: *frames may exceed the sampled count by one
 * per rest, and ms[0..3] over a span that contains that frame are ITS kernels' times, not an average over the span's frames. */
int splat_get_timing(splat_ctx* ctx, double ms[6], uint64_t* frames, int32_t reset);

/* Debug / stage parity: results of the last frame.  splat_get_tile_lists needs a frame rendered WITH a stats pointer
 * (ordinary frames keep the short lists they sort on chip and never write them back: SPLAT_ERR_INVALID then). */
int splat_get_records(splat_ctx* ctx, splat_record* out, uint64_t n);
/* tile_offsets: n_tiles+1 entries (slab-local tiles, row-major); order: n_pairs Gaussian indices,
 * each tile's list in blend order (far -> near). Pass NULL to query sizes via stats. */
int splat_get_tile_lists(splat_ctx* ctx, uint32_t* tile_offsets, uint64_t n_offsets, uint32_t* order,
                         uint64_t n_order);
/* How the last frame was binned: > 0 = one-pass binning (the default), the value being the entries of the key buffer
 * its tiles' regions live in -- every tile owns a region sized from the list it had two frames earlier (x 1.5 + 512 keys),
 * so the buffer holds ~1.6 x the frame's (Gaussian, tile) pairs; a frame whose list outgrows its region is skipped and
 * redone / reported like any frame that outgrows its storage (splat_sync).  0 = two-pass binning (count, scan, emit into
 * exactly sized lists): SPLAT_BUCKETS=0, a caller-fixed pair_capacity, or key buffers that would not fit
 * SPLAT_BUCKET_BYTES (default 128 GiB for all frame slots together).  < 0 without a frame. */
int64_t splat_binning_mode(splat_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: one frame = disjoint TILE-ROW SLABS, one per GPU, every GPU holding the
 * whole scene; the only exchange is one gather of slab pixel rows to the root per frame -- a grouped
 * ncclSend / ncclRecv over xGMI, contiguous rows straight out of each peer's image into the root's.
 * Pixels are independent given the ordered splat list (src/pipelines.rs:147-168), so the gathered frame
 * equals the single-GPU frame byte for byte.  RCCL (librccl.so.1) is loaded on first use.
 * Two forms, same kernels, same gather:
 *   (A) one process per GPU (torchrun / MPI style): splat_comm_* on an ordinary context;
 *   (B) one process, one host thread + context per device: splat_multi_* (ncclCommInitAll).
 * What replaces what: the reference renders the whole frame in one render_to_buffer call
 * (src/pipelines.rs:66-86); euc fans rows out to CPU threads -- these entry points fan tile rows out to GPUs.
 * ------------------------------------------------------------------------------------------------ */
#define SPLAT_UNIQUE_ID_BYTES 128

/* Contiguous tile-row slabs minimising the heaviest slab: row_loads = splat_tile_row_loads() output,
 * row_overhead = fixed cost per tile row in the same unit (pairs).  slabs_out: n_ranks x {row0, row1}.
 * row_loads == NULL: equal split of n_rows.  Deterministic: every rank derives the same partition. */
int splat_slab_partition(const uint64_t* row_loads, int32_t n_rows, int32_t n_ranks, double row_overhead,
                         int32_t* slabs_out);

/* (A) one process per GPU.  Rank 0 calls splat_comm_unique_id and hands the 128 bytes to the other ranks by
 * its own means (a file, a socket, torch.distributed ...); every rank then calls splat_comm_init_rank on its
 * context (collective: ncclCommInitRank on the context's device). */
int splat_comm_unique_id(uint8_t id[SPLAT_UNIQUE_ID_BYTES]);
int splat_comm_init_rank(splat_ctx* ctx, const uint8_t id[SPLAT_UNIQUE_ID_BYTES], int32_t n_ranks, int32_t rank);
/* The partition (n_ranks x {row0,row1}, identical on every rank); also sets this context's own slab. */
int splat_comm_set_slabs(splat_ctx* ctx, const int32_t* slabs);
/* Gather: enqueued on the context's stream behind the frames rendered so far.  d_argb = this rank's w x h
 * device image; afterwards (stream order) the root's image holds every rank's rows. */
int splat_comm_gather(splat_ctx* ctx, void* d_argb, int32_t w, int32_t h, int32_t root);
/* Test hook for one-GPU boxes: with `on`, a SINGLE-rank communicator's gather moves this rank's slab rows through
 * RCCL to itself (ncclSend + ncclRecv to the own rank in one group, on the context's stream) and restores them from
 * what arrived -- the code path, RCCL kernel included, of the multi-rank gather.  The frame is unchanged if RCCL
 * delivered the rows intact.  n_ranks > 1: SPLAT_ERR_INVALID. */
int splat_comm_loopback(splat_ctx* ctx, int32_t on);
void splat_comm_destroy(splat_ctx* ctx);              /* also done by splat_destroy */

/* (B) one process.  devices[i] = HIP ordinal of rank i (rank 0 is the root).  A device may be listed more than
 * once (slabs then share that GPU; RCCL refuses duplicate devices, so rows travel as device-to-device copies
 * ordered by events -- meant for testing the decomposition on a single-GPU box); SPLAT_MULTI_TRANSPORT=peer
 * selects those copies for distinct devices too (hipMemcpyPeerAsync over xGMI). */
typedef struct splat_multi splat_multi;
int splat_multi_create(const splat_config* cfg /* device field ignored; NULL = defaults */, const int32_t* devices,
                       int32_t n_devices, splat_multi** out);
void splat_multi_destroy(splat_multi* m);
const char* splat_multi_last_error(const splat_multi* m);   /* m may be NULL: last create() error */
int splat_multi_upload_scene(splat_multi* m, uint64_t n, const float* pos4, const float* cov3d, const float* opacity,
                             const float* sh);               /* replicated on every device, in parallel */
/* Load-balanced slabs for this camera (count-only pass on the root + splat_slab_partition).  cam == NULL: equal
 * slabs for the target size of the last partition (SPLAT_ERR_INVALID before any frame / balance: the height fixes
 * the tile rows).  The partition stays until the next call or a frame of another target size. */
int splat_multi_balance(splat_multi* m, const splat_camera* cam);
int splat_multi_get_slabs(const splat_multi* m, int32_t* slabs_out /* n_devices x {row0,row1} */);
/* render_to_buffer across the devices: blends the scene onto `argb` (host, in/out, w*h u32).  stats (nullable)
 * = sums over the slabs (a Gaussian that reaches two slabs counts in both). */
int splat_multi_render(splat_multi* m, const splat_camera* cam, uint32_t* argb, splat_stats* stats);
/* Viewer-loop frame (src/main.rs:69-78), device resident: every device clears its slab rows, renders them and
 * sends them to the root's image.  Asynchronous: returns once the frame is queued on every device's thread;
 * splat_multi_sync waits.  The root's image (device memory on devices[0]) is splat_multi_image(). */
int splat_multi_render_frame(splat_multi* m, const splat_camera* cam);
/* Waits for every rank.  SPLAT_ERR_CAPACITY: an asynchronous slab frame outgrew storage sized from earlier frames and
 * was skipped on its device -- the root's image then holds that slab's rows as the gather found them (cleared or
 * stale); the storage has been grown: render the frame again (splat_multi_render_frame may report the same for a loss
 * found while it re-partitions).  Any other error: the first one a rank recorded since the last sync
 * (splat_multi_last_error names the rank). */
int splat_multi_sync(splat_multi* m);
/* The root's image that holds the most recent frame (read it after splat_multi_sync).  With frame overlap 2 the frames of
 * splat_multi_render_frame alternate between two images on every device -- ask again after each frame. */
void* splat_multi_image(splat_multi* m);
/* splat_set_frame_overlap for every rank (default 1).  2: every device keeps two slab images and the frames of
 * splat_multi_render_frame use them in turn, so the compositor (and the row gather) of frame N+1 runs beside frame N's on
 * each device; the partition weighs a tile row's fixed cost for that.  Waits for the frames in flight; the next frame
 * partitions again. */
int splat_multi_set_frame_overlap(splat_multi* m, int32_t n);
int splat_multi_download(splat_multi* m, uint32_t* argb_out, int32_t w, int32_t h);   /* root image -> host (after a sync) */
splat_ctx* splat_multi_ctx(splat_multi* m, int32_t rank);  /* the rank's context (statistics, timing); not to be rendered on directly */

#ifdef __cplusplus
}
#endif
#endif
