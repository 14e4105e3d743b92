// splat_host.hpp -- C++ host-side mirror of the reference crate's public API for the hot path
// (src/lib.rs: camera, gaussians, pipelines), written over the C ABI of include/splat_hip.h.
// Same names, argument meaning and semantics as the Rust items they stand for; where the Rust
// code panics (unwrap) these throw std::runtime_error.
//
//   splat::Camera                    src/camera.rs:4-126
//   splat::Gaussian                  src/gaussians.rs:30-38, 101-113
//   splat::GaussianList              src/gaussians.rs:408-462
//   splat::naive_gaussians()         src/gaussians.rs:319-374
//   splat::load_from_ply()           src/gaussians.rs:246-283, 375-405
//   splat::GaussianSplatPipeline01   src/pipelines.rs:54-87   (AoS, low-pass 0.01)
//   splat::GaussianSplatPipeline02   src/pipelines.rs:172-175, 259-281 (SoA, low-pass 0.3)
#ifndef SPLAT_HOST_HPP
#define SPLAT_HOST_HPP
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "splat_hip.h"

namespace splat {

using Vec3 = std::array<float, 3>;
using Mat4 = std::array<float, 16>;   // column-major, like nalgebra::Matrix4::as_slice()

class Camera {
public:
    // Camera::new(h, w, start_position) -- height first (src/camera.rs:22); default position (0,0,3)
    Camera(float h, float w, const Vec3* start_position = nullptr);
    void compute_matrices();                       // :41-68
    const Mat4& get_view_matrix() const { return view_matrix_; }
    const Mat4& get_project_matrix() const { return projection_matrix_; }
    void update_resolution(float height, float width);
    Vec3 get_htanfovxy_focal() const;              // :84-89
    float get_focal() const;
    void update_pitch_angle(float delta);
    void update_yaw_angle(float delta);
    void update_camera_pose();                     // :103-126
    // the per-frame constants the C ABI takes
    splat_camera constants(float lowpass, int32_t sh_dim = 15) const;

    float h, w;                 // pub
    Vec3 position;              // pub
    bool is_pose_dirty = true;  // pub

private:
    float znear_ = 0.01f, zfar_ = 100.0f, fovy_;
    Vec3 target_{0, 0, 0}, up_{0, -1, 0};
    float yaw_ = 0.0f, pitch_ = 0.0f;
    bool is_intrin_dirty_ = true;
    Mat4 view_matrix_, projection_matrix_;         // identity until compute_matrices (:36-37)
};

struct Gaussian {               // src/gaussians.rs:30-38
    Vec3 position{0, 0, 0};
    Vec3 scale{0, 0, 0};
    float opacity = 0.0f;
    std::array<float, 4> rotation{0, 0, 0, 1};   // nalgebra coords order (i, j, k, w); identity
    std::array<float, 48> sh{};
    std::array<float, 9> cov3d{};                // column-major 3x3, zero until compute_cov3d (:254)
    void compute_cov3d();                        // :101-113 (host arithmetic, one Gaussian)
};

std::vector<Gaussian> naive_gaussians();
std::vector<Gaussian> load_from_ply(const std::string& filename);
struct GaussianList;
// The loader on the fast path: the same decode, activations and recentring, straight into
// the SoA upload buffers, on `threads` host threads (0 = all).  cov3d is left zero (compute_cov3d, K0 on the GPU).
GaussianList load_from_ply_soa(const std::string& filename, int threads = 0);
long long ply_vertex_count(const std::string& filename);      // header only
// Where the loader finds its properties: the splat_ply_layout the device decoder takes (a known name whose type is not
// float is absent; of duplicated names the last wins -- as load_from_ply reads them) and where the vertex rows lie in
// the file.  binary == false (an ascii file): the rows are text and the offsets describe nothing.
struct PlyLayout {
    splat_ply_layout layout;
    bool binary = false;
    uint64_t payload_offset = 0, payload_bytes = 0;
};
PlyLayout ply_layout(const std::string& filename);
// load_from_ply + compute_cov3d + upload as one call whose work is the GPU's: the payload of a binary file is copied to
// the device once, as it is, and decoded, activated, recentred and uploaded there (splat_upload_ply_device); an ascii
// file goes through the host loader and splat_upload_scene.  compute_cov3d == false leaves cov3d zero (Gaussian::new).
// Returns the number of Gaussians; the frames are those of the host path, byte for byte.
uint64_t load_ply_to_gpu(splat_ctx* ctx, const std::string& filename, bool compute_cov3d = true);
// The way back (splat_encode_ply_scene_device, splat_encode_ply_gaussians_device): the RESIDENT scene as PLY vertex rows in
// device memory -- log scales and a quaternion from cov3d, the logit of the opacity, positions and sh with their bits.
// d_index == nullptr: the whole scene (layout.n == the resident n); else row t = Gaussian d_index[t] (layout.n == k).  Positions
// and sh come back bit for bit, covariances and opacities within the error of a float64 decomposition rounded to f32
// (profiles/ply_save_accuracy.json); the loader recentres on every load.  Throws what the C calls refuse.
void encode_ply(splat_ctx* ctx, const splat_ply_layout& layout, void* d_rows_out, uint64_t k = 0, const void* d_index = nullptr,
                void* producer_stream = nullptr);
splat_ply_layout inria_layout(uint64_t n);      // the canonical 62-float file: 248-byte rows, nx ny nz named by no slot
// ... and into a file: the canonical header (binary little endian), the rows encoded into a temporary device buffer and
// copied down once.  d_index == nullptr: the whole scene, k = its n.  Returns the rows written.
uint64_t save_ply_from_gpu(splat_ctx* ctx, const std::string& filename, uint64_t k, const void* d_index = nullptr);
// The resident scene edited in place from DEVICE buffers (splat_update_scene_device, splat_update_gaussians_device):
// `fields` = SPLAT_FIELD_* bits, a buffer whose field is not named may be null.  The whole-field form takes all n rows by
// original index; the indexed form takes k compact rows, row t for Gaussian d_index[t] (u32, distinct).  The order of the
// last upload stays; the frames are those of a fresh upload of the edited arrays.  Throws what the C call refuses.
void update_scene_device(splat_ctx* ctx, uint64_t n, uint32_t fields, const void* d_pos4, const void* d_cov3d,
                         const void* d_opacity, const void* d_sh, void* producer_stream = nullptr);
void update_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, uint32_t fields, const void* d_pos4,
                             const void* d_cov3d, const void* d_opacity, const void* d_sh, void* producer_stream = nullptr);
// ... read back into DEVICE buffers (splat_read_scene_device, splat_read_gaussians_device: the inverses of the two above, same
// layouts, pos4's w = 1, a buffer whose field is not named stays untouched and may be null; duplicate indices are fine), and
// mapped where it lies (splat_transform_scene_device, splat_transform_gaussians_device): m = 3x4 row-major affine map in host
// memory, applied to positions and 3D covariances (A S A^T); opacity and sh keep their bits, sh is not rotated.  The reads
// leave the state kept from frame to frame alone; a transform is an edit like the updates.  Throw what the C calls refuse.
void read_scene_device(splat_ctx* ctx, uint64_t n, uint32_t fields, void* d_pos4, void* d_cov3d, void* d_opacity, void* d_sh);
void read_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, uint32_t fields, void* d_pos4, void* d_cov3d,
                           void* d_opacity, void* d_sh, void* producer_stream = nullptr);
void transform_scene_device(splat_ctx* ctx, const float m[12]);
void transform_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const float m[12], void* producer_stream = nullptr);
// ... and view-dependent colour turned with it (splat_sh_rotation_blocks, splat_rotate_sh_scene_device,
// splat_rotate_sh_gaussians_device): r = 3x3 row-major orthogonal map in host memory (a reflection is fine); bands 1-3 of sh are
// multiplied by the blocks sh_rotation_blocks gives (host only, no context; row-major 3x3, 5x5, 7x7), everything else keeps its
// bits.  Edits like an update of sh alone.  Throw what the C calls refuse (an r that is not orthogonal among it).
void sh_rotation_blocks(const float r[9], float d1[9], float d2[25], float d3[49]);
void rotate_sh_scene_device(splat_ctx* ctx, const float r[9]);
void rotate_sh_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const float r[9], void* producer_stream = nullptr);
// Colour (splat_eval_colours_device, splat_select_colour_device, splat_recolour_scene_device, splat_recolour_gaussians_device).
// eval: the colour each Gaussian is drawn with under cam (cam_pos and sh_dim alone are read), K1's bit for bit, three floats a
// row into d_rgb_out -- all n in original order (d_index null, k == n) or row t = Gaussian d_index[t].  select_colour: that
// colour mapped by q.colour_to_unit into the unit box / ball (splat_colour_query), combined with d_selection by `op` =
// SPLAT_SEL_OP_*; returns the count selected afterwards.  Both read the scene as a selection does.  recolour: rgb' = A rgb + t
// (m = 3x4 row-major in host memory) applied to the sh coefficients in place, whole or for distinct indices: edits like an
// update of sh alone.  Throw what the C calls refuse (a non-finite m among it).
void eval_colours_device(splat_ctx* ctx, const splat_camera& cam, uint64_t k, const void* d_index, void* d_rgb_out,
                         void* producer_stream = nullptr);
uint64_t select_colour_device(splat_ctx* ctx, const splat_colour_query& q, const splat_camera& cam, uint32_t op, void* d_selection,
                              void* producer_stream = nullptr);
void recolour_scene_device(splat_ctx* ctx, const float m[12]);
void recolour_gaussians_device(splat_ctx* ctx, uint64_t k, const void* d_index, const float m[12], void* producer_stream = nullptr);
// A selection by neighbourhood on the resident scene (splat_select_neighbours_device): Gaussian i passes when the number of OTHER
// Gaussians of the source set (d_source: n bytes, nonzero = source, null = all) with centres within `radius` of its own lies in
// [count_min, count_max]; `op` = SPLAT_SEL_OP_* combines that with d_selection (one byte per Gaussian, original index order;
// may be d_source itself).  d_counts_out (n u32, null = not wanted) receives the counts, saturated at count_max + 1;
// d_selection may be null with it.  max_block_pairs bounds the work (0 = no limit; beyond it the C call's SPLAT_ERR_CAPACITY is
// thrown and nothing is written); *block_pairs_out (nullable) receives the number it is compared with.  Returns how many are
// selected after the op.  Floaters: select_neighbours(ctx, r, nullptr, 0, k - 1, SPLAT_SEL_OP_SET, sel, nullptr, limit);
// grow: select_neighbours(ctx, r, sel, 1, 0xFFFFFFFFu, SPLAT_SEL_OP_ADD, sel, nullptr, limit).  Throws what the C call refuses.
uint64_t select_neighbours(splat_ctx* ctx, float radius, const void* d_source, uint32_t count_min, uint32_t count_max, uint32_t op,
                           void* d_selection, void* d_counts_out, uint64_t max_block_pairs, uint64_t* block_pairs_out = nullptr,
                           void* producer_stream = nullptr);
// What lies under up to SPLAT_PICK_MAX_PIXELS pixels of the target of cam (splat_pick_device): pixels_xy = n_pixels (x, y) pairs in
// host memory; per pixel a splat_pick_result into d_results -- n_hits, the front hit and the surface, the first hit nearest
// first at which the float coverage reaches q.coverage_min: what a click should select -- and, with q.max_layers > 0,
// q.max_layers splat_pick_layer rows into d_layers (both device memory).  d_mask: one byte per Gaussian like a selection, null =
// all.  Throws what the C call refuses.
void pick(splat_ctx* ctx, const splat_pick_query& q, const splat_camera& cam, uint32_t n_pixels, const int32_t* pixels_xy,
          const void* d_mask, void* d_results, void* d_layers = nullptr, void* producer_stream = nullptr);
// Gaussians taken out of the resident scene (splat_remove_gaussians_device): d_selection = n bytes like a selection, mode =
// SPLAT_REMOVE_SELECTED (the selected go) or SPLAT_REMOVE_UNSELECTED (they stay); the survivors keep their relative original
// order and are renumbered by rank.  d_index_map_out (n u32, null = not wanted): the new index of every old Gaussian, or
// 0xFFFFFFFF.  Nothing is sorted; the frames are those of a fresh upload of the survivors.  Returns how many are left.  Throws
// what the C call refuses.
uint64_t remove_gaussians_device(splat_ctx* ctx, uint64_t n, const void* d_selection, uint32_t mode = SPLAT_REMOVE_SELECTED,
                                 void* d_index_map_out = nullptr, void* producer_stream = nullptr);
// Gaussians added to the resident scene (splat_append_gaussians_device): m rows in splat_upload_scene_device's four device
// buffers; they get the original indices n .. n+m-1, the resident ones keep theirs and their slots, the new rows are ordered
// among themselves behind them.  The frames are those of a fresh upload of the concatenation.  Returns n + m.  Throws what
// the C call refuses -- a context without a scene among it: that takes an upload.
uint64_t append_gaussians_device(splat_ctx* ctx, uint64_t n, uint64_t m, const void* d_pos4, const void* d_cov3d,
                                 const void* d_opacity, const void* d_sh, void* producer_stream = nullptr);
// The resident scene put into the order a fresh upload of its current values would have (splat_reorder_scene_device): worth
// calling after appends, indexed transforms or updates of positions, and removals.  Returns how many slots hold another
// Gaussian than before; 0: the call has been a read.
uint64_t reorder_scene_device(splat_ctx* ctx);

struct GaussianList {           // src/gaussians.rs:408-416, SoA
    std::vector<float> positions;   // 4 x N (x,y,z,1)
    std::vector<float> scales;      // 3 x N
    std::vector<float> opacities;   // N
    std::vector<float> rotations;   // 4 x N (i,j,k,w)
    std::vector<float> sh;          // 48 x N
    std::vector<float> cov3d;       // 3 x 3N
    size_t num_gaussians = 0;
    // from_vec: gathers the arrays and computes cov3d (:419-440); compute = false keeps each
    // Gaussian's own cov3d (what Pipeline01 renders with)
    static GaussianList from_vec(const std::vector<Gaussian>& v, bool compute = true, splat_ctx* gpu = nullptr);
    void compute_cov3d(splat_ctx* gpu = nullptr);   // :446-462; on the GPU (K0) when a context is given
};

namespace detail {
class PipelineBase {
public:
    ~PipelineBase();
    PipelineBase(const PipelineBase&) = delete;
    PipelineBase& operator=(const PipelineBase&) = delete;
    splat_stats last_stats{};
    // Viewer loop (src/main.rs:69-78) without the stall: stream_frame() == clear + render_to_buffer,
    // queued; the pixels are in `color` after wait_frame(color).  Keep two buffers in flight
    // (pinned ones from alloc_frame make the copy truly asynchronous).
    void wait_frame(const uint32_t* color);
    // `color.clear(0); render_to_buffer(&mut color)` (src/main.rs:73-74) as one synchronous call (splat_render_frame): `color` is
    // written, never read.  pin_frame(color, pixels) once (the reference's buffer lives as long as the window, src/main.rs:62)
    // lets the compositor write straight into it; unpin_frame before the memory goes away.
    static void pin_frame(uint32_t* color, size_t pixels);
    static void unpin_frame(uint32_t* color);
    // The scene is uploaded to the GPU once, at the first frame, and cached (the reference re-reads its
    // public `gaussians` field on every render_to_buffer, src/pipelines.rs:67-79).  After mutating
    // `gaussians` (edits, compute_cov3d after the first frame, ...) call this: the next frame uploads again.
    void invalidate_scene() { uploaded_ = nullptr; }
    // SPLAT_MODE_* flags (include/splat_hip.h) for this pipeline's GPU context; the reference has no such switch and
    // the default (0) is its arithmetic.  Must be called before the first frame (the context is created there).
    void set_mode(int mode);
    static uint32_t* alloc_frame(size_t pixels);
    static void free_frame(uint32_t* p);
protected:
    PipelineBase() = default;
    void render(const GaussianList& g, const Camera& cam, float lowpass, uint32_t* color);
    void render_frame(const GaussianList& g, const Camera& cam, float lowpass, uint32_t* color);
    void stream(const GaussianList& g, const Camera& cam, float lowpass, uint32_t* color);
    void ensure(const GaussianList& g);
    void create_context();
    splat_ctx* ctx_ = nullptr;
    const void* uploaded_ = nullptr;
    int mode_ = 0;
};
}  // namespace detail

class GaussianSplatPipeline01 : public detail::PipelineBase {
public:
    GaussianSplatPipeline01(std::vector<Gaussian> gaussians, Camera camera);
    // Blends onto `color` (w*h u32, 0xAARRGGBB) exactly as src/pipelines.rs:66-86 does.
    void render_to_buffer(uint32_t* color);
    void render_frame_to_buffer(uint32_t* color);   // clear + render_to_buffer, src/main.rs:73-74, in one call (see PipelineBase)
    void stream_frame(uint32_t* color);        // cleared frame, asynchronous (see PipelineBase)
    // The scene straight from a PLY file through load_ply_to_gpu: `gaussians` is left empty, the context holds the scene
    // (invalidate_scene() or a change of `gaussians` goes back to the host copy).  Returns the number of Gaussians.
    uint64_t load_ply_gpu(const std::string& filename, bool compute_cov3d = true);
    std::vector<Gaussian> gaussians;   // pub
    Camera camera;                     // pub
private:
    GaussianList soa_;
};

class GaussianSplatPipeline02 : public detail::PipelineBase {
public:
    GaussianSplatPipeline02(GaussianList gaussians, Camera camera);
    void render_to_buffer(uint32_t* color);    // src/pipelines.rs:260-280
    void render_frame_to_buffer(uint32_t* color);
    void stream_frame(uint32_t* color);
    GaussianList gaussians;            // pub
    Camera camera;                     // pub
};

}  // namespace splat
#endif
