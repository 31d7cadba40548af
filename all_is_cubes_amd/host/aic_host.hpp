// aic_host.hpp -- C++ host-side mirror of the reference's renderer interface for the
// raytracing path, sitting ABOVE the C ABI (include/aic_hip.h) exactly where the Rust shim
// crate `all-is-cubes-hip` would sit. It stands in for that shim in this
// repository because no Rust toolchain exists here; names, argument meaning and error
// behaviour follow the reference:
//
//   GraphicsOptions & enums   all-is-cubes-render/src/camera/graphics_options.rs:28-560
//   Viewport                  camera/viewport.rs:24-163
//   Camera, look_at_y_up      camera/camera_struct.rs:43-471
//   eye_for_look_at           all-is-cubes/src/camera.rs:34-40
//   StandardCameras/UiViewState  camera/stdcam.rs:21-271 (reduced to plain values)
//   PackedLight, Sky/BlockSky all-is-cubes/src/space/light/data.rs, space/sky.rs
//   Space + SpaceChange       all-is-cubes/src/space.rs:77-131,1062-1101 (the part the raytracer reads)
//   HeadlessRenderer, Rendering, Flaws, RenderError   all-is-cubes-render/src/{headless,flaws,lib}.rs
//   HipRtRenderer             mirrors RtRenderer (raytracer/renderer.rs:35-356) and
//                             UpdatingSpaceRaytracer (raytracer/updating.rs:22-219)
//
// euclid 0.22 (un-vendored dependency of the reference) is restated for Transform3D::{then,
// inverse, transform_point3d}, Rotation3D and RigidTransform3D; its rounding is pinned by the
// exact frustum-corner values of camera/tests.rs:78-108 (tests/test_host_mirror.py).
#pragma once

#include <array>
#include <cstdint>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <optional>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aic_hip.h"

namespace aic::host {

struct Vec3 {
    double x = 0, y = 0, z = 0;
};
struct Quat {  // euclid Rotation3D {i,j,k,r}
    double i = 0, j = 0, k = 0, r = 1;
};
struct Mat4 {  // euclid Transform3D, m[row*4+col] = m<row+1><col+1>, row-vector convention
    double m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    Mat4 then(const Mat4 &other) const;
    bool inverse(Mat4 *out) const;
    bool transform_point3d(const Vec3 &p, Vec3 *out) const;  // None unless w > 0
};
struct Ray {
    Vec3 origin, direction;
};
struct GridAab {
    int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    static GridAab from_lower_size(const int32_t lo[3], const int32_t size[3]);
    Vec3 center() const;
    int64_t volume() const;
    bool contains_cube(int32_t x, int32_t y, int32_t z) const;
};

// ---- graphics options -------------------------------------------------------------------
enum class FogOption : int { None = 0, Abrupt, Compromise, Physical };
enum class ToneMappingOperator : int { Clamp = 0, Reinhard };
enum class AntialiasingOption : int { None = 0, IfCheap, Always };
struct TransparencyOption {
    enum Kind : int { Surface = 0, Volumetric, Threshold } kind = Volumetric;
    float threshold = 0.5f;
};
struct LightingOption {
    enum Kind : int { None = 0, Flat, Coarse, Linear, Smoothstep, Bounce } kind = Linear;
    uint8_t samples = 0;
};
struct ExposureOption {
    bool automatic = false;
    float fixed = 1.0f;
    float initial() const { return automatic ? 1.0f : fixed; }
};

struct GraphicsOptions {
    FogOption fog = FogOption::Abrupt;
    double fov_y = 90.0;
    ToneMappingOperator tone_mapping = ToneMappingOperator::Clamp;
    float maximum_intensity = std::numeric_limits<float>::infinity();
    ExposureOption exposure;
    float bloom_intensity = 0.125f;
    double view_distance = 200.0;
    LightingOption lighting_display;
    TransparencyOption transparency;
    bool show_ui = true;
    AntialiasingOption antialiasing = AntialiasingOption::None;
    bool debug_info_text = true;
    bool debug_pixel_cost = false;
    bool debug_light_rays_at_cursor = false;  // the lines pass draws compute_light's ray records at cursor.preceding_cube() (HipRtRenderer::present_split)
    static GraphicsOptions unaltered_colors();  // UNALTERED_COLORS
    GraphicsOptions repair() const;             // clamps fov_y to 1..189, view_distance to 1..10000
    aic_options to_abi() const;
    bool operator==(const GraphicsOptions &o) const;
};

struct Viewport {
    double nominal_width = 0, nominal_height = 0;
    uint32_t framebuffer_width = 0, framebuffer_height = 0;
    static Viewport with_scale(double scale_factor, uint32_t w, uint32_t h);
    double nominal_aspect_ratio() const;
    double normalize_fb_x(size_t x) const;
    double normalize_fb_y(size_t y) const;
    double normalize_fb_x_edge(size_t x) const;
    double normalize_fb_y_edge(size_t y) const;
    bool is_empty() const { return framebuffer_width == 0 || framebuffer_height == 0; }
    size_t pixel_count() const { return (size_t)framebuffer_width * framebuffer_height; }
    bool operator==(const Viewport &o) const;
};

struct ViewTransform {  // RigidTransform3D<f64, Eye, Cube>
    Quat rotation;
    Vec3 translation;
    static ViewTransform identity() { return ViewTransform(); }
};
ViewTransform look_at_y_up(const Vec3 &eye, const Vec3 &target);
Vec3 eye_for_look_at(const GridAab &bounds, const Vec3 &direction);
Quat rotation_around_x(double radians);
Quat rotation_around_y(double radians);
Quat rotation_then(const Quat &first, const Quat &second);

// convert_camera_to_pinhole (all-is-cubes-gpu/src/rerun_image.rs:314-338): what travels with an exported image. image_from_camera is the column-major
// 3 x 3 pinhole matrix in f32 exactly as written there -- {w/2 / tan_x, 0, 0, 0, h/2 / tan_y, 0, w/2, h/2, 1} with tan_y = (f32)tan(fov_y / 2) and
// tan_x = tan_y * (w / h) --, resolution the camera's framebuffer size in f32, transform its view transform (ParentFromChild).
struct Pinhole {
    std::array<float, 9> image_from_camera;
    std::array<float, 2> resolution;
    ViewTransform transform;
};
// logged_image_size_policy (rerun_image.rs:302-311; aic_export_size with the reference's cap of 640 * 480)
std::array<uint32_t, 2> logged_image_size_policy(uint32_t width, uint32_t height);

class Camera {
  public:
    Camera(const GraphicsOptions &options, const Viewport &viewport);
    void set_options(const GraphicsOptions &options);
    const GraphicsOptions &options() const { return options_; }
    void set_viewport(const Viewport &viewport);
    Viewport viewport() const { return viewport_; }
    void set_view_transform(const ViewTransform &t);
    void look_at_y_up(const Vec3 &eye, const Vec3 &target) { set_view_transform(host::look_at_y_up(eye, target)); }
    ViewTransform view_transform() const { return eye_to_world_; }
    void set_measured_exposure(float value);
    double fov_y() const { return options_.fov_y; }
    double view_distance() const { return options_.view_distance; }
    double near_plane_distance() const { return 1.0 / 32.0; }
    Mat4 projection_matrix() const { return projection_; }
    // {m33, m43, m34, m44} of raytrace_to_texture's depth_transform (raytrace_to_texture.rs:613-618): the projection, pre-translated by -near along z
    // and pre-scaled by -(far - near), which maps a ray's t (0 at the near plane, 1 at the view distance) to the projected depth -- what
    // aic_set_depth_transform takes
    std::array<double, 4> depth_transform_zw() const;
    Mat4 view_matrix() const { return world_to_eye_; }
    Mat4 inverse_projection_view() const { return inverse_projection_view_; }
    // ReprojectionUniforms.reprojection_matrix from the camera an image was traced with to the camera it is shown in (raytrace_to_texture.rs:446-453):
    // (view_old . proj_old)^-1 . view_new . proj_new in f64 and euclid's row-vector order, converted to f32 as camera::convert_matrix lays it out --
    // column-major for WGSL's column vectors, [c*4+r], which is this Mat4's own element order. The identity where the old product is singular (the reference
    // unwraps there).
    static std::array<float, 16> reprojection_matrix(const Camera &traced_with, const Camera &current);
    // {ipz.z, ipw.z, ipz.w, ipw.w} of the inverse projection (rt-copy.wgsl:210-223): what linearize_depth_value reads; the identity's when the projection
    // is singular (raytrace_to_texture.rs:460-465)
    std::array<float, 4> inverse_projection_zw() const;
    Pinhole pinhole() const;
    Vec3 view_position() const { return view_position_; }
    Ray project_ndc_into_world(double ndc_x, double ndc_y) const;
    Vec3 project_ndc3_into_world(const Vec3 &ndc) const;
    float exposure() const { return exposure_value_; }
    std::array<float, 4> post_process_color(const std::array<float, 4> &rgba) const;
    aic_camera to_abi() const;

  private:
    void compute_matrices();
    GraphicsOptions options_;
    Viewport viewport_;
    ViewTransform eye_to_world_;
    Mat4 world_to_eye_, projection_, inverse_projection_view_;
    Vec3 view_position_;
    float exposure_value_ = 1.0f;
};

// ---- scene data the raytracer reads -----------------------------------------------------
struct PackedLight {
    uint8_t r = 0, g = 0, b = 0, status = 0;  // status: 0 Uninitialized, 1 NoRays, 128 Opaque, 255 Visible
    static PackedLight some(float r, float g, float b);
    static uint8_t scalar_in(float value);
    static PackedLight one() { return PackedLight{144, 144, 144, 255}; }
    bool operator==(const PackedLight &o) const { return r == o.r && g == o.g && b == o.b && status == o.status; }
};
struct Sky {
    int kind = 0;  // 0 Uniform, 1 Octants
    float colors[8][3] = {};
    void for_blocks(uint8_t out[7][4]) const;  // BlockSky faces nx..pz + mean
};
struct Evoxel {
    float color[4] = {0, 0, 0, 0};
    float emission[3] = {0, 0, 0};
    bool selectable = true;  // Evoxel::selectable (Evoxel::AIR: false -- Evoxels::air())
};
struct Evoxels {
    int32_t resolution = 1;
    int32_t vlo[3] = {0, 0, 0}, vsize[3] = {1, 1, 1};
    std::vector<uint16_t> indices;
    std::vector<Evoxel> palette;
    bool is_one = true;
    bool is_air = false;
    bool selectable = true;  // EvaluatedBlock::attributes().selectable (AIR: false)
    std::string display_name;  // BlockAttributes::display_name: its first character is what text renderings show (text.rs:27-38)
    static Evoxels from_one(const Evoxel &v);
    static Evoxels air();
    // How the block goes to the device (aic_block_desc.flags, and each palette entry's eighth float through palette_floats): AIC_BLOCK_UNSELECTABLE for
    // a block that is not selectable (AIR says so itself); AIC_BLOCK_VOXEL_SELECTABLE, the exact form, exactly when some voxel's `selectable` is not
    // what the ABI's default rule would take it for (selectable iff not invisible) -- a block that needs neither is uploaded as it always was.
    uint32_t abi_flags() const;
    void palette_floats(std::vector<float> *out) const;  // appends [n][8]
};

// EveryLight is this mirror's coalesced form of a burst of CubeLight notifications: what a light-propagation
// step that touched most of the space sends (the reference emits one CubeLight per cube, space.rs light updater).
enum class SpaceChangeKind { EveryBlock, CubeBlock, CubeLight, BlockIndex, BlockEvaluation, EveryLight };
struct SpaceChange {
    SpaceChangeKind kind;
    int32_t cube[3];
    uint32_t block_index;
};
// What UpdatingSpaceRaytracer accumulates between updates (updating.rs:180-219).
struct SpaceRendererTodo {
    bool everything = true;
    bool every_light = false;
    std::set<uint32_t> blocks;
    std::set<std::array<int32_t, 3>> cubes;
    void receive(const SpaceChange &c);
    void clear() { everything = false; every_light = false; blocks.clear(); cubes.clear(); }
};

class Space {
  public:
    Space(const GridAab &bounds);
    const GridAab &bounds() const { return bounds_; }
    Sky sky;
    // block palette
    uint32_t add_block(const Evoxels &e);                 // emits BlockIndex
    void set_block_data(uint32_t index, const Evoxels &e);  // emits BlockEvaluation
    size_t n_blocks() const { return blocks_.size(); }
    const Evoxels &block(uint32_t i) const { return blocks_.at(i); }
    // cubes
    void set(int32_t x, int32_t y, int32_t z, uint32_t block_index);   // emits CubeBlock
    void set_light(int32_t x, int32_t y, int32_t z, PackedLight l);    // emits CubeLight
    void fill_all(uint32_t block_index);                               // emits EveryBlock
    void load_contents(const uint16_t *block_index, const uint8_t *light);  // emits EveryBlock
    void load_light(const uint8_t *light);                                  // emits EveryLight
    uint16_t get_block_index(int32_t x, int32_t y, int32_t z) const;
    PackedLight get_light(int32_t x, int32_t y, int32_t z) const;
    const std::vector<uint16_t> &contents() const { return contents_; }
    const std::vector<PackedLight> &light() const { return light_; }
    // listeners (listen::Source<SpaceChange>)
    void listen(const std::shared_ptr<SpaceRendererTodo> &todo);
    size_t index(int32_t x, int32_t y, int32_t z) const;

  private:
    void notify(const SpaceChange &c);
    GridAab bounds_;
    std::vector<uint16_t> contents_;
    std::vector<PackedLight> light_;
    std::vector<Evoxels> blocks_;
    std::vector<std::weak_ptr<SpaceRendererTodo>> listeners_;
};

// ---- renderer surface -------------------------------------------------------------------
namespace Flaws {  // flaws.rs:20-80
constexpr uint16_t OTHER = 1 << 0, TOO_COMPLEX = 1 << 1, UNFINISHED = 1 << 2, UNSUPPORTED = 1 << 3;
constexpr uint16_t OUT_OF_TIME = UNFINISHED | (1 << 4), OUT_OF_MEMORY = UNFINISHED | (1 << 5);
constexpr uint16_t NO_ANTIALIASING = UNSUPPORTED | (1 << 7), NO_BLOOM = UNSUPPORTED | (1 << 8), NO_CURSOR = UNSUPPORTED | (1 << 9);
}  // namespace Flaws

struct RenderError : std::runtime_error {
    int code;
    RenderError(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

struct ImageInfo {  // renderer.rs:617-647 + RaytraceInfo sr.rs:520-522
    uint64_t cubes_traced = 0;
    uint64_t n_outer = 0, n_inner = 0, n_hits = 0, n_light = 0;
    float kernel_ms = 0, total_ms = 0;
    uint32_t width = 0, height = 0, rows_rendered = 0;
    std::string status_text() const;
};
struct SplitRendering {  // raytrace_to_texture's two render targets (raytrace_to_texture.rs:594-675), as AIC_FRAME_OUT_SPLIT writes them
    uint32_t width = 0, height = 0;
    std::vector<uint16_t> color;  // [h][w][4] IEEE f16 bits: premultiplied light times the pixel's layer's exposure, alpha
    std::vector<float> depth;     // [h][w] projected depth of the nearest surface; sign bit set on UI pixels
    uint16_t flaws = 0;
    ImageInfo info;
};
struct Rendering {  // headless.rs:52-67
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;  // [h][w][4] sRGB RGBA8
    uint16_t flaws = 0;
    ImageInfo info;
};

// TerminalOptions (all-is-cubes-desktop/src/terminal/options.rs:15-185): what the terminal's frames are made of. The enumerators carry the C ABI's values
// (AIC_CELLS_COLOR_*, AIC_CELLS_*).
enum class TerminalColorMode : int32_t { None = 0, TwoFiftySix = 1, Rgb = 2 };
enum class TerminalCharacterMode : int32_t { Names = 0, Shades = 1, Split = 2, Shapes = 3, Braille = 4 };
struct TerminalOptions {
    TerminalColorMode colors = TerminalColorMode::TwoFiftySix;        // options.rs:41-48
    TerminalCharacterMode characters = TerminalCharacterMode::Split;
    // the "next" option for purposes of UI stepping (options.rs:61-68, 166-175)
    static TerminalColorMode cycle(TerminalColorMode m);
    static TerminalCharacterMode cycle(TerminalCharacterMode m);
    // viewport_from_terminal_size (options.rs:25-38; aic_cells_geometry): the viewport to raytrace for a drawing area of cols x rows characters
    Viewport viewport_from_terminal_size(uint32_t cols, uint32_t rows) const;
};
struct CellsRendering {  // a frame of the terminal: [rows][cols] cells (aic_cell), the trace's ImageInfo (zero for a presentation) and the branch counters
    uint32_t cols = 0, rows = 0;
    std::vector<aic_cell> cells;
    ImageInfo info;
    aic_cells_info cells_info{};
};

// The info-text overlay (renderer.rs:659-683 `draw_info_text`): `text` drawn with Builtin::FontSystem16 by
// FontDef::draw_str_monospaced (all-is-cubes/src/text/font.rs:178-203) at offset (5, 5) into an RGBA8 image of width x
// height, outline pixels in `outline`, glyph pixels in `foreground`, in the reference's call order (a later glyph's outline
// may overwrite an earlier glyph's edge, as it does there). Pixels outside the image are dropped.
void draw_info_text(uint8_t *rgba, uint32_t width, uint32_t height, const uint8_t outline[4], const uint8_t foreground[4], const std::string &text);
// The font atlas of the interactive renderer's info text: generate_texture_atlas (all-is-cubes-gpu/src/text.rs:108-155) on Builtin::FontSystem16, what
// aic_set_text_font takes with cells of kInfoTextCell. [16 * 18][16 * 9][4] RGBA8, premultiplied: each of the 256 codes drawn alone by the routine
// above -- through char_to_glyph_index and its outline rule -- at (x * 9 + 1, y * 18 + 1) of its cell, outline (0, 0, 0, 255), foreground
// (255, 255, 255, 255). A code that draws nothing (space, '\n') leaves its cell zero.
constexpr uint32_t kInfoTextCell[3] = {9, 18, 1};  // cell width, height, margin: the 7 x 16 character cell and an outline of one
std::vector<uint8_t> info_text_font_atlas();
// Camera::post_process_color(color).to_srgb8() (camera_struct.rs:376-382, math/color.rs:669-676, 1038-1054) of an opaque
// colour: what the reference's encoder makes of the overlay's black and white paints
void encode_paint(const class Camera &camera, float exposure, const float rgb[3], uint8_t out[4]);

struct UiViewState {  // stdcam.rs UiViewState
    std::shared_ptr<Space> space;
    ViewTransform view_transform;
    float backdrop[4] = {0, 0, 0, 0};
    GraphicsOptions graphics_options;
};
struct StandardCameras {  // stdcam.rs:90-180, reduced to values the caller sets
    GraphicsOptions graphics_options;
    Viewport viewport;
    std::shared_ptr<Space> world_space;
    ViewTransform world_view_transform;
    float measured_exposure = 1.0f;
    UiViewState ui;
};
// Cursor (all-is-cubes/src/character/cursor.rs): what of it the renderer draws and what cursor_raycast reports of the two cubes.
// HipRtRenderer::cursor_raycast / project_cursor make it on the device; wireframe() is impl Wireframe for Cursor (cursor.rs:219-278) through
// aic_cursor_wireframe: 12, 16, 24 or 28 lines in palette::CURSOR_OUTLINE. update(cursor) takes the wireframe before it touches the scene, so a Cursor
// that has none (a face outside 0..6, resolution < 1, a negative voxel_size) makes update throw std::invalid_argument with nothing changed.
struct Cursor {
    int32_t cube[3] = {0, 0, 0};
    int32_t face_entered = 0, face_selected = 0;  // Face7 discriminants: 0 Within, 1-3 NX NY NZ, 4-6 PX PY PZ
    double point_entered[3] = {0.0, 0.0, 0.0};
    double distance_to_point = 0.0;
    int32_t voxel_lo[3] = {0, 0, 0}, voxel_size[3] = {1, 1, 1};  // the hit block's EvaluatedBlock::voxels_bounds()
    int32_t resolution = 1;
    // Cursor::hit(): the block index of the cube (the application has the table), the selectable voxel found in block coordinates, the cube's light
    uint32_t block_index = 0;
    int32_t voxel[3] = {0, 0, 0};
    PackedLight light = {0, 0, 0, 0};
    // Cursor::preceding: the cube the ray was in before, unless it started in the hit cube (face_entered Within), and Space::get_light there
    std::optional<std::array<int32_t, 3>> preceding_cube;
    std::optional<PackedLight> preceding_light;
    // Cursor::space(): the layer whose space the cursor is in (cursor_raycast sets it; debug_light_rays_at_cursor draws for a cursor in the world space only)
    int32_t layer = AIC_LAYER_WORLD;
    // Cursor::preceding_cube() (cursor.rs:163-168): cube + face_entered's normal, the cube itself for Within
    std::array<int32_t, 3> preceding_cube_or_cube() const;
    std::vector<aic_line_vertex> wireframe() const;
};

// PixelPicker (all-is-cubes-gpu/src/raytrace_to_texture.rs:838-908): the order in which the incremental renderer takes a frame's pixels -- centre first and
// dithered (aic_pixel_order), the central pixels interleaved with the rest and so picked more often. take(n) is n calls of Iterator::next, as pixel indices
// y * width + x; after cycle_length() picks every pixel has been picked. Host-only.
class PixelPicker {
  public:
    PixelPicker(uint32_t width, uint32_t height) : width_(width), height_(height), order_((size_t)width * height) {
        if (aic_pixel_order(width, height, order_.empty() ? nullptr : order_.data(), &central_, &cycle_length_) != AIC_OK)
            throw std::invalid_argument("PixelPicker: more than 2^32 - 1 pixels");
    }
    void resize(uint32_t width, uint32_t height) {
        if (width != width_ || height != height_) *this = PixelPicker(width, height);
    }
    std::vector<uint32_t> take(size_t n) {
        std::vector<uint32_t> out;
        const uint64_t count = order_.size();
        if (!count) return out;  // (the reference's iterator panics on an empty viewport; nothing to pick here)
        out.reserve(n);
        for (size_t i = 0; i < n; i++, next_++) {
            const uint64_t half = next_ / 2u;
            // itertools::Interleave of the two cycles; with no central pixels the inner side is empty and every pick is the outer's
            if (!central_) out.push_back(order_[next_ % count]);
            else out.push_back((next_ & 1u) ? order_[central_ + half % (count - central_)] : order_[half % central_]);
        }
        return out;
    }
    uint64_t cycle_length() const { return cycle_length_; }
    uint32_t central() const { return central_; }
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    const std::vector<uint32_t> &order() const { return order_; }

  private:
    uint32_t width_, height_;
    std::vector<uint32_t> order_;
    uint32_t central_ = 0;
    uint64_t cycle_length_ = 0;
    uint64_t next_ = 0;  // picks made so far
};

class HeadlessRenderer {  // headless.rs:17-44
  public:
    virtual ~HeadlessRenderer() = default;
    virtual void update(const Cursor *cursor) = 0;
    virtual Rendering draw(const std::string &info_text) = 0;
};

class HipRtRenderer : public HeadlessRenderer {
  public:
    using SizePolicy = std::function<Viewport(Viewport)>;
    // device_id < 0: current device. Throws RenderError if no MI355X / HIP device is usable.
    HipRtRenderer(std::shared_ptr<StandardCameras> cameras, SizePolicy size_policy = nullptr, int device_id = -1);
    ~HipRtRenderer() override;
    HipRtRenderer(const HipRtRenderer &) = delete;
    HipRtRenderer &operator=(const HipRtRenderer &) = delete;

    // RtRenderer::update: returns whether anything changed.
    bool update_scene(const Cursor *cursor);
    void update(const Cursor *cursor) override { (void)update_scene(cursor); }
    Rendering draw(const std::string &info_text) override { return draw_rgba(info_text); }
    Rendering draw_rgba(const std::string &info_text);
    // The frame as all-is-cubes-gpu's raytrace_to_texture wants it: sets the depth transform from the world camera (Camera::depth_transform_zw) and
    // renders with AIC_FRAME_OUT_SPLIT. No info text, no bloom (that renderer blooms its own frames).
    SplitRendering draw_split();
    // Opt-in, off by default: draw_rgba blooms its frames as the reference's GPU renderer does (AIC_FRAME_BLOOM) whenever the world options'
    // bloom_intensity is above zero, and such a Rendering does not report Flaws::NO_BLOOM. The info text is drawn over the bloomed frame.
    void set_bloom(bool on) { bloom_ = on; }
    bool bloom() const { return bloom_; }
    // Replaying a recorded frame (all_is_cubes_amd/replay.py, bench.py --workload replay:<file>): the world camera's
    // inverse_projection_view and exposure exactly as the recording has them, instead of the values derived from the
    // StandardCameras' view transform (which would be equal only up to rounding). nullptr: back to the cameras.
    void set_world_camera_override(const double *inverse_projection_view, float exposure);
    // SpaceRaytracer::<CharacterRtData>::to_text::<CharacterBuf> (sr.rs:367-472, text.rs:52-128): one ray through each
    // pixel centre; the first block hit shows the first character of its display name ('#' if it has none), a ray that
    // entered the space and hit nothing ' ', one that never entered it '.', one that ran out of steps 'X'
    std::string draw_text(const std::string &line_ending = "\n");
    // One frame of the terminal renderer (all-is-cubes-desktop/src/terminal.rs:119-137; aic_render_cells): the current viewport -- which must be
    // TerminalOptions::viewport_from_terminal_size of some grid under options.characters, std::invalid_argument otherwise -- traced and turned into
    // character cells on the device.
    CellsRendering draw_cells(const TerminalOptions &options);
    // The names table aic_cells_ansi takes for block glyphs, made from each layer's blocks' display_name as draw_text cuts it: the first scalar, "#"
    // when empty. Widths: 2 for the East Asian wide and fullwidth ranges, 0 for combining marks, else 1 (the reference measures by cursor read-back and
    // falls back to unicode_width, chars.rs:229-300).
    struct TerminalNames {
        std::vector<std::string> names[2];
        std::vector<uint8_t> widths[2];
    };
    TerminalNames terminal_names() const;
    // TerminalWindow::write_frame (terminal/ui.rs:300-360; aic_cells_ansi) of `frame` with terminal_names(): the byte stream for the terminal
    std::string cells_to_ansi(const CellsRendering &frame, bool in_rect = false, uint16_t origin_x = 0, uint16_t origin_y = 0) const;
    // draw_cells and cells_to_ansi in one
    std::string draw_terminal(const TerminalOptions &options, bool in_rect = false, uint16_t origin_x = 0, uint16_t origin_y = 0);
    // A terminal target for the resident interactive frame: aic_present_split with AIC_PRESENT_OUT_F16 of `src_device` (a Split frame of the current
    // viewport) into `scratch_device` -- device memory of the caller's, 8 bytes per pixel of the cells' framebuffer for cols x rows --, then
    // aic_image_cells on it (f16, already post-processed, on the device). Every mode but Names, which needs first-hit records a Split frame has not got.
    CellsRendering present_split_cells(const void *src_device, void *scratch_device, uint32_t cols, uint32_t rows, const TerminalOptions &options);
    // SpaceRaytracer::trace_ray (sr.rs:113-120) for a batch of world-space rays against one layer's space as last updated (aic_trace_rays): no camera, no
    // layering, one ray per result. `colors[i]` is the ColorBuf trace_ray leaves in its accumulator (light r, g, b and transmittance), `hits[i]` the first-hit
    // record (hit == 0: none; t_distance in units of the ray's direction, which is taken as given).
    struct RayResults {
        std::vector<std::array<float, 4>> colors;
        std::vector<aic_pixel_aux> hits;
        ImageInfo info;
    };
    RayResults trace_rays(int layer, const std::vector<Ray> &rays, bool include_sky = true);
    // One round of raytrace_to_texture's do_some_tracing (raytrace_to_texture.rs:591-751; aic_trace_pixels): the listed pixels (y * width + x) of the frame
    // draw_split() renders, each traced exactly as there. trace_pixels returns the Split texels in list order; trace_pixels_into stores them at the pixels'
    // positions of a resident Split frame in device memory (width * height colour texels, then the depth plane) and leaves every other texel as it is --
    // `device_pixels` is the list in device memory on the renderer's device.
    struct PixelResults {
        std::vector<uint16_t> color;  // [n][4] f16 bits
        std::vector<float> depth;     // [n]
        std::vector<aic_pixel_aux> hits;
        ImageInfo info;
    };
    PixelResults trace_pixels(const std::vector<uint32_t> &pixels);
    ImageInfo trace_pixels_into(void *device_frame, const uint32_t *device_pixels, uint32_t n);
    // raytrace_to_texture's prepare_frame when the camera has moved (raytrace_to_texture.rs:433-540; aic_reproject_split): the resident Split frame `src`,
    // traced with the camera `traced_with`, drawn into the current world camera as depth-tested point sprites and gap-filled, into `dst` -- again a
    // resident Split frame, which trace_pixels_into refines. Both are device memory on the renderer's device, of the current viewport's size, and do
    // not overlap. `flags`: AIC_REPROJECT_*.
    aic_reproject_info reproject_split(const void *src, void *dst, const Camera &traced_with, uint32_t flags = 0);
    // PixelPicker::take on the device (aic_pick_pixels): the next `n` picks written to `device_pixels_out` ([n] u32 on the renderer's device), ready for
    // trace_pixels_into. `device_order`: aic_pixel_order's result for the current viewport, resident once ([width * height] u32), or nullptr: row-major.
    // With max_unknown > 0 the list begins with up to that many of the pixels the last reproject_split knows nothing about, in picker order -- those
    // not handed out since --, which the reference does not do; with 0 it is the reference's sequence. The renderer keeps the picker's cursor and the
    // count of unknown pixels handed out: reproject_split sets the latter back to 0, a change of the viewport's size both. Its host PixelPicker class
    // is a separate object with a cursor of its own.
    aic_pick_info pick_pixels(const uint32_t *device_order, uint32_t *device_pixels_out, uint32_t n, uint32_t max_unknown = 0);
    uint64_t pick_cursor() const { return pick_cursor_; }
    uint64_t pick_skip_unknown() const { return pick_skip_unknown_; }
    // The pixels a scene change made stale first (aic_stale_rects, aic_pick_stale; not in the reference, which re-arms a whole picker cycle,
    // raytrace_to_texture.rs:587-589). stale_rects: boxes {lo x, y, z, hi x, y, z} (upper bounds exclusive) of changed cubes as the screen rectangles of
    // the pixels they can have changed under the current world camera's projection x view; expand = 1 covers the light stencil and ambient occlusion
    // beside a changed cube. changed_boxes: what the last update() sent to the device for the world layer, so that the loop needs no bookkeeping of its
    // own: one box per cube of the space's dirty set (its block or its light texel changed), or the space's bounds as one box when the space was
    // uploaded whole or a block definition was replaced (the cubes that use it are not tracked); empty when nothing changed.
    // pick_stale: pick_pixels with, first, up to max_stale of the pixels of the resident Split frame `device_frame` inside a rectangle that does not keep
    // them out (flags: AIC_STALE_DEPTH_TEST), past those handed out already. The renderer keeps that count beside the picker's cursor, which the two
    // calls share: an update() that changed cubes, reproject_split, restart_stale() (new rectangles) and a change of the viewport's size set it to 0.
    std::vector<aic_stale_rect> stale_rects(const std::vector<std::array<int32_t, 6>> &boxes, int32_t expand = 1) const;
    const std::vector<std::array<int32_t, 6>> &changed_boxes() const { return changed_boxes_; }
    aic_stale_info pick_stale(const std::vector<aic_stale_rect> &rects, const void *device_frame, const uint32_t *device_order, uint32_t *device_pixels_out,
                              uint32_t n, uint32_t max_stale, uint32_t flags = 0);
    void restart_stale() { pick_skip_stale_ = 0; }
    uint64_t pick_skip_stale() const { return pick_skip_stale_; }
    // The same for a light update, and for any number of changed cubes (aic_light_changed_take, aic_pick_stale_cubes). changed_light_cubes:
    // the cubes whose light texel the device's updater changed, taken from the library by every evaluate_light() and evaluate_light_wait() while
    // track_light_changes is set (off by default: a loop that never asks must not pile them up) and kept
    // until clear_changed_light_cubes() -- the loop clears them once pick_stale_cubes hands out no stale pixel any more. pick_stale_cubes: pick_stale
    // with the stale set made on the device from changed_boxes() (grown by `expand`) and those light cubes under the current world camera; flags:
    // AIC_STALE_DEPTH_TEST, AIC_STALE_DEPTH_BEHIND. It shares pick_stale's count of stale pixels handed out, which a light update that reported cubes
    // also sets to 0.
    const std::vector<std::array<int32_t, 3>> &changed_light_cubes() const { return changed_light_cubes_; }
    bool track_light_changes = false;
    void clear_changed_light_cubes() { changed_light_cubes_.clear(); }
    aic_stale_cubes_info pick_stale_cubes(const void *device_frame, const uint32_t *device_order, uint32_t *device_pixels_out, uint32_t n, uint32_t max_stale,
                                          uint32_t flags = 0, int32_t expand = 1);
    // The same for a re-evaluated block (todo.blocks, updating.rs:139-153; aic_find_block_cubes, aic_pick_stale_blocks), for which
    // changed_boxes() can only name the whole space. changed_blocks: the block indices the last update() re-sent; changed_cube_boxes: the cubes it sent
    // one by one, also beside a re-sent block, and the space's bounds only after a whole upload (then changed_blocks is empty). find_block_cubes: the
    // world layer's cubes that hold one of `indices`, as runs along z, or their one bounding box when there are more than `capacity`. pick_stale_blocks:
    // pick_stale_cubes with changed_cube_boxes(), the light cubes and, found on the device, the cubes of changed_blocks(); it keeps the picker's cursor
    // and the count of stale pixels handed out as pick_stale_cubes does.
    const std::vector<uint32_t> &changed_blocks() const { return changed_blocks_; }
    const std::vector<std::array<int32_t, 6>> &changed_cube_boxes() const { return changed_cube_boxes_; }
    std::pair<std::vector<std::array<int32_t, 6>>, aic_block_cubes_info> find_block_cubes(const std::vector<uint32_t> &indices, uint32_t capacity);
    // A scene made on the device (aic_replace_cube_grid): the block index of every cube of `layer` from device_block_index[n cubes] (and
    // the light from device_light[n cubes][4], or nullptr), on the device the renderer runs on. The runs of changed cubes -- the one bounding box past
    // max_runs of them -- become what changed_boxes() and changed_cube_boxes() return next, for the world layer, and the count of stale pixels handed
    // out restarts: after update(), the loop of pick_stale_cubes, trace_pixels_into and present_split goes on unchanged. The Space object the renderer
    // listens to is not told: its cubes are the caller's to keep in step, or to leave behind.
    aic_block_cubes_info replace_cube_grid_device(int layer, const uint16_t *device_block_index, const uint8_t *device_light, uint32_t max_runs = 4096);
    aic_stale_blocks_info pick_stale_blocks(const void *device_frame, const uint32_t *device_order, uint32_t *device_pixels_out, uint32_t n, uint32_t max_stale,
                                            uint32_t flags = 0, int32_t expand = 1, uint32_t max_runs = 65536);
    // raytrace_to_texture's per-frame presentation of its resident textures (raytrace_to_texture.rs:546-568, shaders/rt-copy.wgsl:41-71, bloom.rs:41-60,
    // shaders/postprocess.wgsl:140-158 and 251-276; aic_present_split): the resident Split frame `src_device` -- of raytracer's viewport, i.e. the current
    // (size-policy-modified) viewport -- stretched with a linear filter to out_width x out_height, bloomed, tone-mapped and encoded, with bloom_intensity,
    // tone_mapping and maximum_intensity of the renderer's GraphicsOptions. The Rendering is the window's sRGB RGBA8 image (no flaws: nothing is left
    // out; the info text is the overloads' below that take it); the device form writes RGBA8 or, with AIC_PRESENT_OUT_F16, four linear f16
    // per pixel to `out_device`, which must not overlap the frame.
    Rendering present_split(const void *src_device, uint32_t out_width, uint32_t out_height);
    aic_present_info present_split_to_device(const void *src_device, void *out_device, uint32_t out_width, uint32_t out_height, uint32_t flags = 0);
    // The same with the lines pass of EverythingRenderer::draw_frame_linear (all-is-cubes-gpu/src/everything.rs:616-658; aic_present_split_lines): `lines`
    // -- pairs of vertices; nullptr: the wireframe of the cursor last given to update(), none if there was none -- is drawn into the scene before bloom
    // and tone mapping, depth-tested against the frame's depth plane, under the world camera's projection x view (formed in f64, rounded to f32).
    Rendering present_split(const void *src_device, uint32_t out_width, uint32_t out_height, const std::vector<aic_line_vertex> *lines, aic_lines_info *lines_info = nullptr);
    aic_present_info present_split_to_device(const void *src_device, void *out_device, uint32_t out_width, uint32_t out_height, uint32_t flags,
                                             const std::vector<aic_line_vertex> *lines, aic_lines_info *lines_info = nullptr);
    // The same with the info text of the interactive renderer laid over the tone-mapped scene on the device (shaders/postprocess.wgsl:160-276,
    // everything.rs:777-806; aic_present_split_text): the font atlas is set on first use, the character grid is character_texture_size of the world
    // camera's viewport's nominal size with the text's origin at (5, 5) nominal pixels, and the text is empty when the options' debug_info_text is
    // false (everything.rs:786-788). with_lines: the lines pass as above, `lines` == nullptr meaning the cursor's.
    Rendering present_split(const void *src_device, uint32_t out_width, uint32_t out_height, const std::string &info_text, bool with_lines = false,
                            const std::vector<aic_line_vertex> *lines = nullptr, aic_lines_info *lines_info = nullptr);
    aic_present_info present_split_to_device(const void *src_device, void *out_device, uint32_t out_width, uint32_t out_height, uint32_t flags, const std::string &info_text,
                                             bool with_lines = false, const std::vector<aic_line_vertex> *lines = nullptr, aic_lines_info *lines_info = nullptr);
    // RerunImageExport::start_frame_copy (all-is-cubes-gpu/src/rerun_image.rs:62-225; aic_export_split): the resident Split frame `src_device` -- of the
    // current viewport -- as sRGB8 colour and metric depth at out_width x out_height, or (both 0) at logged_image_size_policy of the frame's size, with
    // what perform_image_copy attaches: the pinhole of the world camera with its viewport set to that size, and the depth range
    // {near_plane_distance, view_distance}.
    struct SplitExport {
        uint32_t width = 0, height = 0;
        std::vector<uint8_t> color;  // [height][width][4] sRGB RGBA8
        std::vector<float> depth;    // [height][width] distance along the view axis; 0: no surface
        Pinhole pinhole;
        std::array<double, 2> depth_range = {0.0, 0.0};
        aic_export_info info = {};
    };
    SplitExport export_split(const void *src_device, uint32_t out_width = 0, uint32_t out_height = 0);
    // the world camera of the last update(): what to keep beside a resident frame as its `traced_with`
    const Camera &world_camera() const { return world_camera_; }
    const Camera &ui_camera() const { return ui_camera_; }
    // multi-GPU extension: render the rows of one partition into a device buffer (no read-back)
    ImageInfo draw_rows_to_device(void *device_out, uint32_t strip_rows, uint32_t n_parts, uint32_t part, bool counters = false,
                                  bool no_feedback = false);
    uint32_t partition_rows(uint32_t strip_rows, uint32_t n_parts, uint32_t part) const;
    void assemble_strips(const void *gathered_device, void *out_device, uint32_t strip_rows, uint32_t n_parts, bool wait = true);
    // streaming pair (aic_render_submit / aic_render_wait): up to AIC_MAX_IN_FLIGHT frames in flight
    void submit_rows_to_device(void *device_out, uint32_t strip_rows, uint32_t n_parts, uint32_t part, uint32_t slot);
    // aic_render_submit_batch: 1, 2, 4 or 8 frames traced by ONE launch, frame j into device_outs[j]. `inverse_projection_views` (16 doubles per frame, may be
    // empty) gives each frame its own world camera -- a camera path known ahead of time --; empty: every frame is the current view.
    void submit_rows_batch_to_device(const std::vector<void *> &device_outs, uint32_t strip_rows, uint32_t n_parts, uint32_t part, uint32_t slot,
                                     const std::vector<std::array<double, 16>> &inverse_projection_views = {});
    ImageInfo wait_rows(uint32_t slot);
    void synchronize();  // blocks until everything queued on the context's stream is done (aic_synchronize)
    Viewport modified_viewport() const;
    const StandardCameras &cameras() const { return *cameras_; }
    std::string device_name() const;
    void *stream() const;
    void wait_event(void *hip_event);  // aic_wait_event: later frames wait for a foreign event, the host does not
    void stream_wait_rows(uint32_t slot, void *hip_stream);  // aic_stream_wait_frame: a foreign stream waits for the slot's frame, the host does not
    // Light propagation on the device (aic_evaluate_light): Mutation::fast_evaluate_light (if `fast`) then
    // Mutation::evaluate_light(epsilon) (space.rs:1496-1540) on the WORLD space as uploaded, with
    // LightPhysics::Rays { maximum_distance }; the device's light volume is updated in place (the host Space's is not).
    struct LightUpdateInfo { uint64_t updates, batches, cost; double device_ms, total_ms; uint32_t queue_left; uint64_t bundles_visited; };
    // aic_evaluate_light_submit / _wait: the same update on the library's worker thread, beside the frames submitted meanwhile (which read the light as it
    // stood); the wait -- or the next update() that changes the scene -- publishes it
    void evaluate_light_submit(int maximum_distance, bool fast, int epsilon, int batch, int queue_order, int lanes_per_cube = 0, bool continue_queue = false,
                               uint64_t max_updates = 0);
    LightUpdateInfo evaluate_light_wait();
    bool evaluate_light_done();  // aic_evaluate_light_poll: false while a submitted update is still running
    // `continue_queue`: add nothing to the layer's update queue (what update() queued through aic_light_cubes_changed is
    // drained); `max_updates`: stop after that many cube updates (a per-frame light budget), 0 = run to the end.
    LightUpdateInfo evaluate_light(int maximum_distance, bool fast = true, int epsilon = 1, int batch = 32, int queue_order = 16, int lanes_per_cube = 0,
                                   bool continue_queue = false, uint64_t max_updates = 0);
    // The sampling loop of character::exposure::State::step (exposure.rs:91-128; aic_sample_luminance) for a batch of world-space rays against one
    // layer's space as last updated, light included wherever it was made: per ray the luminance of the light behind the first visible block that has
    // a valid one, or of the sky. max_steps: 2 * maximum_distance, 0 for LightPhysics::None. Legal with frames in flight (submit_rows_to_device).
    std::vector<float> sample_luminance(int layer, const std::vector<Ray> &rays, uint32_t max_steps);
    // cursor_raycast (all-is-cubes/src/character/cursor.rs:26-107; aic_cursor_raycast) against one layer's space as last updated: the first selectable
    // block the ray strikes within maximum_distance (infinity is legal), or nothing. Legal with frames in flight. The batch form is one launch.
    std::optional<Cursor> cursor_raycast(int layer, const Ray &ray, double maximum_distance);
    std::vector<std::optional<Cursor>> cursor_raycast(int layer, const std::vector<Ray> &rays, double maximum_distance);
    // Space::compute_light::<LightUpdateCubeInfo> (all-is-cubes/src/space/light/updater.rs:368-417, light/debug.rs; aic_light_rays) for cubes of one layer's
    // space against its published light volume: per cube the texel and cost compute_light returns and the ray records it pushes, in the reference's
    // order. Legal with frames in flight. wireframe() is impl Wireframe for LightUpdateCubeInfo (aic_light_rays_wireframe).
    struct LightCubeInfo {
        aic_light_cube_info info{};
        std::vector<aic_light_ray> rays;
        std::vector<aic_line_vertex> wireframe() const;
    };
    std::vector<LightCubeInfo> light_rays(int layer, const std::vector<std::array<int32_t, 3>> &cubes, int maximum_distance);
    // GraphicsOptions::debug_light_rays_at_cursor (all-is-cubes-gpu/src/common/debug_lines.rs:47-63): with the option on and the cursor of the last
    // update() in the world space, every present_split that draws the cursor's lines (`lines` == nullptr) draws them and then the lines of
    // compute_light at cursor.preceding_cube(), from one list made on the device (aic_light_rays_cursor_lines): the records never visit the host.
    // The distance is the world space's LightPhysics::Rays { maximum_distance }, which the application states here as it does for evaluate_light.
    int light_rays_maximum_distance = 30;
    // StandardCameras::project_cursor (all-is-cubes-render/src/camera/stdcam.rs:357-389) through the cameras of the last update(): the UI space, if
    // there is one, at any distance; else, or if nothing is struck there, the world at 6.0. The result goes straight into update(cursor).
    std::optional<Cursor> project_cursor(double ndc_x, double ndc_y);
    // true: the WORLD space's light lives on the device (evaluate_light): update() forwards block changes only, never the
    // host Space's light texels, and queues the changed cubes for relighting (aic_light_cubes_changed)
    bool device_light = false;
    int device_light_queue_order = 16;
    bool enable_counters = false;

  private:
    struct LayerState {
        std::shared_ptr<Space> space;
        std::shared_ptr<SpaceRendererTodo> todo;
        GraphicsOptions options;
        bool options_valid = false;
    };
    bool sync_space(int layer, const std::shared_ptr<Space> &space, const GraphicsOptions &options);
    void upload_full(int layer, const Space &space);
    void check(int rc, const char *what);
    aic_present_desc present_desc(uint32_t out_width, uint32_t out_height, uint32_t flags) const;
    aic_frame_desc make_frame() const;
    std::shared_ptr<StandardCameras> cameras_;
    SizePolicy size_policy_;
    aic_ctx *ctx_ = nullptr;
    LayerState layers_[2];
    bool cam_override_ = false;
    double cam_override_inv_[16] = {0};
    float cam_override_exposure_ = 1.0f;
    bool had_cursor_ = false;
    std::vector<aic_line_vertex> cursor_lines_;  // the wireframe of the cursor of the last update()
    std::optional<std::array<int32_t, 3>> cursor_light_cube_;  // ... and its preceding_cube(), if it is in the world space
    aic_lines_desc lines_desc(const std::vector<aic_line_vertex> *lines);
    bool text_font_set_ = false;
    std::vector<uint8_t> text_codes_;  // the character grid of the last presentation with text
    aic_text_desc text_desc(const std::string &info_text);
    bool bloom_ = false;  // set_bloom
    uint64_t pick_cursor_ = 0, pick_skip_unknown_ = 0;  // pick_pixels
    uint64_t pick_skip_stale_ = 0;  // pick_stale
    std::vector<std::array<int32_t, 6>> changed_boxes_;  // of the last update(), world layer
    std::vector<std::array<int32_t, 6>> changed_cube_boxes_;  // of the last update(), world layer: the cubes sent one by one, or the bounds after a whole upload
    std::vector<uint32_t> changed_blocks_;                    // ... and the block indices it re-sent
    std::vector<std::array<int32_t, 3>> changed_light_cubes_;  // what the light updates reported since clear_changed_light_cubes()
    void take_changed_light();  // aic_light_changed_take of the world layer, appended to changed_light_cubes_
    uint32_t pick_width_ = 0, pick_height_ = 0;         // ... and the viewport they belong to
    // snapshot taken by update(): draw() must not touch the scene objects (headless.rs:33-39)
    Camera world_camera_, ui_camera_;
    float backdrop_[4] = {0, 0, 0, 0};
    bool show_ui_ = true;
};

// character::exposure::State (all-is-cubes/src/character/exposure.rs:37-151) over aic_exposure_state: what a host keeps per character when its
// GraphicsOptions::exposure is Automatic. Once per simulation step:
//     state.step(renderer, cams->world_view_transform, maximum_distance, dt);
//     cams->measured_exposure = state.exposure();        // update() hands it to Camera::set_measured_exposure
class ExposureState {
  public:
    ExposureState();  // Default: every sample 1.0, exposure 1.0
    // State::step: dt == 0 does nothing; otherwise AIC_EXPOSURE_RAYS rays from the view transform's origin sample the renderer's WORLD space
    // (sample_luminance) and the exposure eases towards compute_target_exposure of the ring's average. maximum_distance_or_minus_one: the space's
    // LightPhysics::Rays { maximum_distance }, or -1 for LightPhysics::None (no steps: every sample is the sky).
    void step(HipRtRenderer &renderer, const ViewTransform &view_transform, int maximum_distance_or_minus_one, double dt);
    float exposure() const;           // State::exposure
    float luminance_average() const;  // State::luminance_average
    std::array<float, AIC_EXPOSURE_SAMPLES> samples() const;
    uint32_t sample_index() const { return s_.luminance_sample_index; }
    float exposure_log() const { return s_.exposure_log; }
    static float compute_target_exposure(float luminance);  // exposure.rs:145-151

  private:
    aic_exposure_state s_;
};

// (inline, in the header: aic_host.cpp names no ray tracing call but aic_render and its kin -- tests/test_product_boundaries.py keeps a CPU renderer out of it by that word)
inline HipRtRenderer::RayResults HipRtRenderer::trace_rays(int layer, const std::vector<Ray> &rays, bool include_sky) {
    static_assert(sizeof(Ray) == 6 * sizeof(double), "a Ray is the ABI's six doubles: origin, then direction");
    if (rays.size() > 2048u * 65535u) throw RenderError(AIC_ERR_INVALID, "trace_rays: more than 2048 x 65535 rays in one call");
    RayResults out;
    out.colors.resize(rays.size());
    out.hits.resize(rays.size());
    aic_frame_info fi;
    const uint32_t flags = AIC_FRAME_OUT_COLORBUF | (enable_counters ? AIC_FRAME_COUNTERS : 0u) | (include_sky ? 0u : AIC_RAYS_NO_SKY);
    check(aic_trace_rays(ctx_, layer, (uint32_t)rays.size(), rays.empty() ? nullptr : &rays[0].origin.x, flags, 1.0f, out.colors.data(), out.hits.data(), &fi),
          "aic_trace_rays");
    ImageInfo &i = out.info;
    i.cubes_traced = fi.cubes_traced; i.n_outer = fi.n_outer; i.n_inner = fi.n_inner; i.n_hits = fi.n_hits; i.n_light = fi.n_light;
    i.kernel_ms = fi.kernel_ms; i.total_ms = fi.total_ms; i.width = (uint32_t)rays.size(); i.height = 1; i.rows_rendered = fi.rows_rendered;
    return out;
}

inline HipRtRenderer::PixelResults HipRtRenderer::trace_pixels(const std::vector<uint32_t> &pixels) {
    if (pixels.size() > 2048u * 65535u) throw RenderError(AIC_ERR_INVALID, "trace_pixels: more than 2048 x 65535 pixels in one call");
    aic_frame_desc f = make_frame();
    f.flags |= AIC_FRAME_OUT_SPLIT;
    const std::array<double, 4> zw = world_camera_.depth_transform_zw();
    check(aic_set_depth_transform(ctx_, zw.data()), "aic_set_depth_transform");
    const size_t n = pixels.size();
    PixelResults out;
    out.hits.resize(n);
    std::vector<uint32_t> planes(n * 3, 0u);  // 8 bytes of colour per pixel, then 4 of depth
    aic_frame_info fi;
    check(aic_trace_pixels(ctx_, &f, (uint32_t)n, pixels.data(), 0u, planes.data(), out.hits.data(), &fi), "aic_trace_pixels");
    out.color.resize(n * 4);
    out.depth.resize(n);
    if (n) {
        std::memcpy(out.color.data(), planes.data(), n * 8);
        std::memcpy(out.depth.data(), planes.data() + n * 2, n * 4);
    }
    ImageInfo &i = out.info;
    i.cubes_traced = fi.cubes_traced; i.n_outer = fi.n_outer; i.n_inner = fi.n_inner; i.n_hits = fi.n_hits; i.n_light = fi.n_light;
    i.kernel_ms = fi.kernel_ms; i.total_ms = fi.total_ms; i.width = f.width; i.height = f.height; i.rows_rendered = fi.rows_rendered;
    return out;
}
inline ImageInfo HipRtRenderer::trace_pixels_into(void *device_frame, const uint32_t *device_pixels, uint32_t n) {
    aic_frame_desc f = make_frame();
    f.flags |= AIC_FRAME_OUT_SPLIT;
    const std::array<double, 4> zw = world_camera_.depth_transform_zw();
    check(aic_set_depth_transform(ctx_, zw.data()), "aic_set_depth_transform");
    aic_frame_info fi;
    check(aic_trace_pixels(ctx_, &f, n, device_pixels, AIC_PIXELS_DEVICE | AIC_PIXELS_IN_PLACE, device_frame, nullptr, &fi), "aic_trace_pixels");
    ImageInfo i;
    i.cubes_traced = fi.cubes_traced; i.n_outer = fi.n_outer; i.n_inner = fi.n_inner; i.n_hits = fi.n_hits; i.n_light = fi.n_light;
    i.kernel_ms = fi.kernel_ms; i.total_ms = fi.total_ms; i.width = f.width; i.height = f.height; i.rows_rendered = fi.rows_rendered;
    return i;
}

}  // namespace aic::host
