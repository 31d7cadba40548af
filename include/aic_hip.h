/*
 * aic_hip.h -- C ABI of the MI355X-native voxel raytracer (libaic_hip.so).
 *
 * This is the drop-in boundary for ONE path of kpreid/all-is-cubes v0.10.0: the CPU
 * raytracer behind `HeadlessRenderer` / `RtRenderer`
 * (all-is-cubes-render/src/headless.rs:17-44, src/raytracer/renderer.rs:35-356).
 * The reference has no FFI for this path (all-is-cubes-render is #![forbid(unsafe_code)],
 * lib.rs:21); these entry points are what a new `all-is-cubes-hip` crate implementing
 * `HeadlessRenderer` would bind (see INTEGRATION.md for the Rust `extern "C"` block).
 * Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *  - plain C, plain pointers and sizes; no C++ / torch types.
 *  - every function returning `int` returns an AIC_* status; aic_last_error() gives text.
 *  - host buffers passed in are copied before the call returns; the caller keeps ownership.
 *  - a context is bound to one HIP device (one process per GPU); it may be moved between
 *    threads but used by one thread at a time (`&mut self`; RtRenderer is Send+Sync,
 *    renderer.rs:696-698).
 *  - all grids are Z-major: index = ((x-lo.x)*size.y + (y-lo.y))*size.z + (z-lo.z)
 *    (all-is-cubes-base/src/math/vol.rs:988-1023).
 */
#ifndef AIC_HIP_H
#define AIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIC_ABI_VERSION 3

/* status codes */
#define AIC_OK 0
#define AIC_ERR_INVALID 1      /* bad argument (maps to a panic/assert in the reference) */
#define AIC_ERR_NO_DEVICE 2    /* no usable HIP device */
#define AIC_ERR_OOM 3          /* device allocation failed => Flaws::OUT_OF_MEMORY-style degradation */
#define AIC_ERR_DEVICE 4       /* HIP runtime error / device lost => RenderError (lib.rs:46-54) */
#define AIC_ERR_UNSUPPORTED 5

/* layers (camera/stdcam.rs:21-28 `Layers { world, ui }`) */
#define AIC_LAYER_WORLD 0
#define AIC_LAYER_UI 1

/* Flaws bits reported in aic_frame_info.flaws (all-is-cubes-render/src/flaws.rs:20-80) */
#define AIC_FLAW_UNSUPPORTED 1u   /* an option was substituted (Flaws::UNSUPPORTED). Reported by nothing at present: LightingOption::Bounce, which
                                   * rounds 1-3 rendered as Linear (graphics_options.rs:460-467), is traced as the reference does since round 4 */
#define AIC_FLAW_NO_BLOOM 2u      /* renderer.rs:293-297 */

/* block descriptor flags */
#define AIC_BLOCK_ONE 1u  /* EvoxelsInner::One(voxel): resolution 1, palette[pal_off] is the voxel */
#define AIC_BLOCK_AIR 2u  /* block == AIR (TracingCubeData.always_invisible, sr.rs:543-564) */
/* What aic_cursor_raycast needs of a block beyond its picture (no trace, light or exposure kernel reads either; a caller that sets neither bit uploads
 * what it always did):
 * AIC_BLOCK_UNSELECTABLE: EvaluatedBlock::attributes().selectable == false. A block with AIC_BLOCK_AIR is unselectable with or without this bit.
 * AIC_BLOCK_VOXEL_SELECTABLE: the eighth float of each of this block's palette entries is Evoxel::selectable, exactly 1.0f (selectable) or +0.0f (not);
 * any other pattern is rejected with AIC_ERR_INVALID by aic_upload_space / aic_replace_block(s). This is the EXACT form. Without the bit the eighth float
 * stays an ignored pad and a voxel counts as selectable iff it is not invisible (alpha != 0 or emission != 0): an APPROXIMATION whose one sure case is
 * the commonest unselectable voxel, Evoxel::AIR -- an invisible voxel that is selectable, or a visible one that is not, needs the bit. */
#define AIC_BLOCK_UNSELECTABLE 4u
#define AIC_BLOCK_VOXEL_SELECTABLE 8u

/* One Space block-palette entry = `TracingBlock.voxels: Evoxels`
 * (sr.rs:568-587; all-is-cubes/src/block/eval/voxel_storage.rs:199-227). 48 bytes. */
typedef struct aic_block_desc {
    int32_t resolution;  /* 1..128, power of two (resolution.rs:18-31) */
    int32_t vlo[3];      /* stored voxel volume: lower corner ... */
    int32_t vsize[3];    /* ... and size; may be smaller than resolution^3 (outside => AIR) */
    uint32_t vox_off;    /* offset in u16 elements into aic_space_desc.voxels */
    uint32_t pal_off;    /* offset in entries into aic_space_desc.palette */
    uint32_t pal_len;
    uint32_t flags;      /* AIC_BLOCK_* */
    int32_t reserved;
} aic_block_desc;

/* Full snapshot of one Space = the inputs of `SpaceRaytracer::new` (sr.rs:64-88). */
typedef struct aic_space_desc {
    int32_t lo[3];
    int32_t size[3];
    const uint16_t *block_index; /* [n cubes] `Space` contents (space.rs:77) */
    const uint8_t *light;        /* [n cubes][4] PackedLight::as_texel r,g,b,status (light/data.rs:160-170) */
    uint32_t n_blocks;
    const aic_block_desc *blocks;
    const uint16_t *voxels;      /* pool of palette indices, Z-major per block */
    uint64_t n_voxels;
    const float *palette;        /* pool [n_palette][8]: Evoxel color rgba, emission rgb, pad (Evoxel::selectable for the entries of a block flagged
                                  * AIC_BLOCK_VOXEL_SELECTABLE). Every component of colour and emission must be what the
                                  * reference's Rgba / Rgb can hold (PositiveSign<f32> x 3 + ZeroOne<f32>, math/color.rs:288-314): not NaN,
                                  * not negative, alpha <= 1 -- anything else is rejected with AIC_ERR_INVALID by aic_upload_space /
                                  * aic_replace_block(s) (since round 3; the kernel's compositing and its table powf rely on it). A block
                                  * with pal_len > 0 (or AIC_BLOCK_ONE) needs a non-null palette, one with voxels a non-null voxel pool. */
    uint64_t n_palette;
    int32_t sky_kind;            /* 0 Sky::Uniform(sky[0]); 1 Sky::Octants (sky.rs:16-21) */
    float sky[8][3];             /* Rgb = PositiveSign<f32> x 3: not NaN, not negative (rejected with AIC_ERR_INVALID otherwise; -0.0 is kept as +0.0, as in
                                  * the reference's type, restricted_number.rs:283 -- palette components likewise) */
    uint8_t block_sky[7][4];     /* Sky::for_blocks(): faces nx,ny,nz,px,py,pz then mean, as texels (sky.rs:45-82) */
} aic_space_desc;

/* The subset of GraphicsOptions the raytracer honours (camera/graphics_options.rs:28-152). */
typedef struct aic_options {
    int32_t fog;              /* FogOption: 0 None, 1 Abrupt, 2 Compromise, 3 Physical */
    int32_t transparency;     /* TransparencyOption: 0 Surface, 1 Volumetric, 2 Threshold */
    float threshold;          /* Threshold(t) */
    int32_t lighting;         /* LightingOption: 0 None, 1 Flat, 2 Coarse, 3 Linear, 4 Smoothstep, 5 Bounce */
    int32_t bounce_samples;
    int32_t antialiasing;     /* AntialiasingOption: 0 None, 1 IfCheap, 2 Always */
    int32_t debug_pixel_cost;
    int32_t tone_mapping;     /* ToneMappingOperator: 0 Clamp, 1 Reinhard */
    float maximum_intensity;  /* may be +inf */
    float bloom_intensity;    /* reported back as AIC_FLAW_NO_BLOOM, unless a frame asks for AIC_FRAME_BLOOM */
    double view_distance;     /* already `repair()`ed: clamped to 1..10000 (graphics_options.rs:194-198) */
} aic_options;

/* One Camera as the kernel needs it (camera/camera_struct.rs:43-77). */
typedef struct aic_camera {
    double inverse_projection_view[16]; /* euclid order m11..m44; Camera.inverse_projection_view (412-416) */
    float exposure;                     /* Camera::exposure() (365-367): a PositiveSign<f32> -- a frame with a negative or NaN exposure is rejected */
    int32_t reserved;
} aic_camera;

/* Which rows of the frame this context renders: rows are grouped into strips of
 * `strip_rows`; strip s belongs to part (s % n_parts). n_parts = 1 renders everything.
 * (Image rows are independent work items in the reference too: renderer.rs:537-555.) */
typedef struct aic_partition {
    uint32_t strip_rows;
    uint32_t n_parts;
    uint32_t part;
    uint32_t reserved;
} aic_partition;

typedef struct aic_frame_desc {
    uint32_t width, height;      /* framebuffer size after size_policy (renderer.rs:226-233) */
    aic_camera world;            /* used if a world space is uploaded */
    aic_camera ui;               /* used if a UI space is uploaded */
    float backdrop[4];           /* UiViewState.backdrop; all-zero = none (renderer.rs:235-253) */
    aic_partition partition;
    uint32_t flags;              /* AIC_FRAME_* */
    uint32_t tuning;             /* 0 = the library's choices. Otherwise (measurement and tests; ABI 3 -- until then these were environment
                                  * variables the library read per frame: AIC_TILE_QUEUES, AIC_SUPER_SHIFT, AIC_XCHG_TILES):
                                  *   bits 0-3   number of tile queues the frame's work tiles are dealt to, 1..8 (0: one per XCD)
                                  *   bits 4-8   super-block edge in macro tiles, log2, PLUS ONE (0: the largest power of two within an eighth of
                                  *              the image height)
                                  *   bits 9-10  AIC_VARIANT_*: which production variant of the trace kernel runs (0: by the frame's size)
                                  * aic_frame_info.variant / .tile_queues report what ran. Any value gives the same image. */
} aic_frame_desc;

#define AIC_TUNE_QUEUES_SHIFT 0
#define AIC_TUNE_SUPER_SHIFT 4
#define AIC_TUNE_VARIANT_SHIFT 9
/* production variants of the trace kernel (aic_frame_desc.tuning to ask for one, aic_frame_info.variant to learn which ran) */
#define AIC_VARIANT_AUTO 0       /* request only: the exchanging variant for a frame of several tiles per resident wave */
#define AIC_VARIANT_PLAIN 1      /* persistent waves, per-lane refill */
#define AIC_VARIANT_EXCHANGING 2 /* ... and lanes exchanged between the waves of a workgroup through a pool of parked rays */
#define AIC_VARIANT_RECORDING 3  /* report only: the variant that writes aic_pixel_aux records / the four byte counters (AIC_FRAME_AUX, AIC_FRAME_COUNTERS) */

#define AIC_FRAME_COUNTERS 1u /* also accumulate n_outer/n_inner/n_hits/n_light */
#define AIC_FRAME_AUX 2u      /* also write the per-pixel aic_pixel_aux records */
/* float output instead of sRGB RGBA8: the output buffer holds [rows][width] float[4] (16 bytes per pixel) */
#define AIC_FRAME_OUT_LINEAR 8u    /* Rgba::from(ColorBuf) (raytracer_components.rs:141-163): linear r,g,b,a before exposure and
                                    * tone mapping -- what a float framebuffer wants */
#define AIC_FRAME_OUT_COLORBUF 16u /* the ColorBuf itself: premultiplied light r,g,b and transmittance
                                    * (raytracer_components.rs:20-39; raytrace_to_texture.rs:638-655 reads exactly this) */
#define AIC_FRAME_NO_FEEDBACK 32u  /* neither use nor record the tile-cost feedback (the order in which this context hands out
                                    * work tiles, learnt from its previous frame of the same shape and camera): a "cold" single
                                    * frame, as the first frame of any sequence is */
/* Bloom (ABI 3, backward compatible): the reference's GPU renderer blooms every frame, raytraced ones included (all-is-cubes-gpu
 * raytrace_to_texture.rs:644-661, bloom.rs:41-60, mip_ping.rs:301-420); the raytracer itself reports AIC_FLAW_NO_BLOOM (renderer.rs:293-297).
 * With this flag, and world options with bloom_intensity > 0, the frame's ColorBuf goes into context-owned scratch (per slot, allocated on
 * first use: 16 bytes per pixel plus the mip chain, about 5 MB at 1080p), through the dual-filter chain (3 repetitions of up to 6 f16 levels)
 * and is mixed into the scene before the tone map; the caller's buffer receives that RGBA8 and the frame does not report AIC_FLAW_NO_BLOOM.
 * Mix in straight alpha: x = ps_mul(c, exposure) (1 - i) + (B / a) i, c and a = Rgba::from(ColorBuf), then the usual tone map and sRGB8
 * encode; a pixel with a = 0 is unchanged (DESIGN.md "Bloom" has the chain and why). Honoured by aic_render, aic_render_submit / _wait and
 * aic_render_submit_batch / _wait_batch; aic_frame_info.kernel_ms then covers the trace AND the bloom, and aic_render_wait /
 * aic_stream_wait_frame order behind the composite. At bloom_intensity 0 the flag changes nothing.
 * AIC_ERR_INVALID with AIC_FRAME_OUT_LINEAR / AIC_FRAME_OUT_COLORBUF; AIC_ERR_UNSUPPORTED with a partition of n_parts > 1 (bloom needs the
 * whole frame), in aic_trace_patches and in every aic_multi_* render. The context stays usable after either. */
#define AIC_FRAME_BLOOM 64u
/* Split (ABI 3, backward compatible): the two texels all-is-cubes-gpu's raytrace_to_texture stores per pixel from its `Split { color, depth, layer }`
 * accumulator (raytrace_to_texture.rs:594-675, 922-977). The output buffer (8-byte aligned) holds two planes, one after the other, 12 bytes per pixel:
 *   colour [rows][width] of four IEEE f16: (l0 e, l1 e, l2 e, a), (l0, l1, l2, a) = ColorBuf::into_premultiplied_rgba of the pixel's (mean) ColorBuf
 *          -- the one AIC_FRAME_OUT_COLORBUF writes, a = clamp(1 - t, 0, 1) --, e = the exposure of the pixel's layer (frame->ui.exposure, frame->world.exposure,
 *          1.0 for no layer), plain f32 products converted as half::f16::from_f32 does (to nearest even, overflow to infinity);
 *   depth  [rows][width] of f32, at byte offset rows * width * 8: the projected depth of the nearest surface, negative (sign bit set: -0.0 at depth 0) for
 *          a UI pixel or a pixel of no layer.
 * rows = the rows the partition selects, compacted as for RGBA8. A sample's layer is that of the first hit after which its ColorBuf is no longer
 * invisible (exception hits carry the layer whose options they are made with: the sky the layer traced, the backdrop the UI's, the NO_WORLD_TO_SHOW paint
 * the world's), the pixel's the first sample's that has one. A sample's depth is the minimum t_distance over its hits that carry one (the UI trace, then the
 * world trace, each in its own camera's ray units; +inf for the sky and after a paint), the pixel's the minimum over its samples (DepthBuf::mean,
 * accum.rs:284-297). Then, in f64, d = clamp(depth, 0, 1), z = d zw[0] + zw[1], w = d zw[2] + zw[3] (euclid's transform_point3d_homogeneous of (0, 0, d))
 * and the value is (float)(z / w), times -1.0f for a UI pixel or none; zw: aic_set_depth_transform.
 * Honoured by aic_render (host or device target; with AIC_FRAME_AUX too), aic_render_submit / _wait and aic_render_submit_batch / _wait_batch, with any
 * partition; the frame is traced by the recording variant (AIC_VARIANT_RECORDING), whatever `tuning` asks for. AIC_ERR_INVALID with AIC_FRAME_OUT_LINEAR,
 * AIC_FRAME_OUT_COLORBUF or AIC_FRAME_BLOOM; AIC_ERR_UNSUPPORTED in aic_trace_patches and every aic_multi_* render; aic_trace_rays has no such output (bit 9 of
 * its flags asks for a kernel variant). The context stays usable after a rejection. */
#define AIC_FRAME_OUT_SPLIT 512u
#define AIC_FRAME_PIXEL_CENTERS 4u /* one ray through each pixel centre, Viewport::normalize_fb_x/_y (viewport.rs:89-99),
                                    * as the text renderer casts them (sr.rs:400-472); default: the image path's patch
                                    * centres / antialiasing points (renderer.rs:424-451) */

/* `RaytraceInfo` / `ImageInfo` (sr.rs:508-537; renderer.rs:617-647) + kernel timing. */
typedef struct aic_frame_info {
    uint64_t cubes_traced; /* RaytraceInfo.cubes_traced summed over the rendered pixels */
    uint64_t n_outer;      /* in-bounds cube-grid lookups */
    uint64_t n_inner;      /* in-bounds voxel lookups */
    uint64_t n_hits;       /* surfaces converted to light (Surface::to_light returned Some) */
    uint64_t n_light;      /* light texel fetches */
    float kernel_ms;       /* HIP-event time of the trace kernel on the context's stream (with AIC_FRAME_BLOOM: the trace and the bloom) */
    float total_ms;        /* launch + read-back wall time of the call */
    uint32_t rows_rendered;
    uint32_t flaws;        /* AIC_FLAW_* */
    uint32_t variant;      /* AIC_VARIANT_*: the trace kernel variant that traced the frame's world pass (ABI 3) */
    uint32_t tile_queues;  /* tile queues the frame's work tiles were dealt to (0: the single counter -- patch and ray batches, orthographic views) */
} aic_frame_info;

/* Optional per-pixel record (N4 "other accumulators": first-hit id and depth): the first
 * Hit carrying a Position that reached the accumulator (raytracer/hit.rs:23-123). */
typedef struct aic_pixel_aux {
    int32_t hit;           /* 0 none, 1 surface */
    int32_t cube[3];
    int32_t voxel[3];
    int32_t resolution;
    int32_t face;          /* Face7 discriminant */
    int32_t block_index;   /* index into the block table of the layer named by `layer` */
    uint32_t cubes_traced; /* steps taken by this pixel's rays */
    uint32_t layer;        /* AIC_LAYER_WORLD / AIC_LAYER_UI: the layer the first hit belongs to */
    double t_distance;
} aic_pixel_aux;

typedef struct aic_ctx aic_ctx;

/* --- lifetime ------------------------------------------------------------------------ */
/* replaces: RtRenderer::new (renderer.rs:65-81). device_id < 0 selects the current device. */
aic_ctx *aic_create(int device_id, int *status);
void aic_destroy(aic_ctx *ctx);
const char *aic_last_error(const aic_ctx *ctx);
int aic_abi_version(void);
/* name of the HIP device the context is bound to (for Info / logging) */
int aic_device_name(const aic_ctx *ctx, char *buf, uint32_t buf_len);

/* --- scene snapshot: RtRenderer::update -> UpdatingSpaceRaytracer::update -------------- */
/* replaces: SpaceRaytracer::new on SpaceChange::EveryBlock / first update
 * (updating.rs:107-126; sr.rs:64-88, prepare_cubes 543-549).
 * Limits (AIC_ERR_INVALID beyond them): the kernel addresses the cube grid + voxel volumes (2 bytes per element) and the light volume (4 bytes per cube)
 * by 32-bit byte offsets, so cubes + voxels < 2^31 and cubes < 2^30 (a 1024^3 space is one cube too many); at most 65536 blocks. */
int aic_upload_space(aic_ctx *ctx, int layer, const aic_space_desc *space);
/* replaces: `rts.<layer> = None` (renderer.rs:134-135). */
int aic_clear_space(aic_ctx *ctx, int layer);
/* replaces: the `todo.cubes` scatter of UpdatingSpaceRaytracer::update (updating.rs:146-166)
 * fed by SpaceChange::{CubeBlock, CubeLight} (updating.rs:201-219). block_index or light may be
 * NULL to leave that field unchanged. xyz are absolute cube coordinates. */
int aic_update_cubes(aic_ctx *ctx, int layer, uint32_t n, const int32_t *xyz, const uint16_t *block_index,
                     const uint8_t *light);
/* replaces: a bulk SpaceChange::CubeLight burst after a light-propagation step (config 5):
 * re-uploads the whole light volume ([n cubes][4]). */
int aic_update_light_volume(aic_ctx *ctx, int layer, const uint8_t *light);
/* replaces: the `todo.blocks` re-evaluation of UpdatingSpaceRaytracer::update (updating.rs:128-145)
 * for SpaceChange::{BlockIndex, BlockEvaluation}: replaces or appends (index == n_blocks) one
 * palette entry. `voxels`/`palette` hold only this block's data (desc offsets are ignored). */
int aic_replace_block(aic_ctx *ctx, int layer, uint32_t index, const aic_block_desc *desc, const uint16_t *voxels,
                      const float *palette);
/* The same for a batch of blocks under ONE wait for the frames in flight and one synchronisation (a tick that
 * re-evaluates many animated blocks: updating.rs:128-145 runs once per changed block index). A block whose new voxel
 * volume and palette fit its current ranges is overwritten in place; one that outgrew them is appended, and the pools
 * are re-packed on the device once the ranges left behind exceed a quarter of a pool. */
int aic_replace_blocks(aic_ctx *ctx, int layer, uint32_t n, const uint32_t *indices, const aic_block_desc *descs,
                       const uint16_t *const *voxels, const float *const *palettes);
/* Re-pack the layer's voxel and palette pools now (done automatically by aic_replace_block(s) past a threshold). */
int aic_compact(aic_ctx *ctx, int layer);
/* replaces: the graphics_options DynSource (updating.rs:24,68-73). */
int aic_set_options(aic_ctx *ctx, int layer, const aic_options *options);
/* The depth transform of AIC_FRAME_OUT_SPLIT frames: zw = {m33, m43, m34, m44} of the caller's depth_transform (raytrace_to_texture.rs:613-618: the
 * camera's projection, pre-translated by -near along z and pre-scaled by -(far - near)), euclid names. Default {1, 0, 0, 1}: the plane is the linear depth.
 * Waits for the frames in flight; the frames submitted from then on use it. AIC_ERR_INVALID for a component that is not finite. */
int aic_set_depth_transform(aic_ctx *ctx, const double zw[4]);

/* --- drawing: RtRenderer::draw_rgba / HeadlessRenderer::draw --------------------------- */
/* replaces: RtRenderer::draw_rgba -> trace_scene_to_image_impl (renderer.rs:282-308, 516-556):
 * out_rgba8 receives the rows selected by frame->partition, compacted in increasing row order,
 * as sRGB RGBA8 row-major (headless.rs:52-67). `out_is_device` != 0: out_rgba8 is a device
 * pointer on the context's device (no read-back; used for the RCCL gather). */
int aic_render(aic_ctx *ctx, const aic_frame_desc *frame, void *out_rgba8, int out_is_device, aic_frame_info *info);
/* Streaming pair for frame sequences (the reference's recording loop renders frame after frame,
 * all-is-cubes-desktop/src/record.rs:97-113): aic_render_submit queues a frame on slot
 * 0..AIC_MAX_IN_FLIGHT-1 and returns at once; aic_render_wait blocks until that slot's frame is in
 * `out_device` and reports it. With several frames in flight the next frame's trace starts filling the
 * GPU while the previous frame's last rays finish; a frame of many tiles that is submitted while others are in flight is launched on a part of the
 * chip (a third with three others in flight, a quarter from four on), so that the frames in flight are resident side by side -- same pixels and counts,
 * a higher frame rate, a longer life of each frame; a frame submitted with nothing else in flight takes the whole chip. out_device must be a device pointer; the
 * AIC_FRAME_AUX flag is ignored here (use aic_render). Scene updates that change what a frame in flight
 * reads (aic_upload_space, aic_update_cubes, aic_replace_blocks, aic_compact) wait for every
 * frame in flight first (aic_set_options waits for nothing: a frame carries the options it was submitted under); aic_update_light_volume and aic_evaluate_light do NOT: they write the other half of the
 * light double buffer beside the frames in flight (which keep the half they were given) and only wait for a frame
 * still reading that other half.
 * Slots 0..7 are made with the context; a higher slot gets its stream and events when it is first used.
 * A frame of no pixels (a partition's part that has no rows) queues nothing and occupies its slot like any other until it is waited for: the wait
 * reports zeros, and until then a second submit on the slot, and on slot 0 the work that runs there, is refused.
 * "The frame is in out_device" is all aic_render_wait (and aic_render with a device target) waits for: behind the frame the slot's
 * stream still prepares the slot's next frame (the frame's cost record becomes a tile order, counters are cleared -- microseconds of
 * work private to the slot). Work the caller orders behind the frame with aic_stream_wait_frame, or issues after the wait returns,
 * never has to wait for that. aic_render_wait does NOT drain the slot's stream: call aic_synchronize before handing aic_stream() to
 * other code that assumes it idle.
 * Slots are HIP streams; the runtime runs streams that share one of its GPU_MAX_HW_QUEUES hardware queues (4 when unset) one behind the other.
 * The library does not touch that variable: the host's environment decides (INTEGRATION.md "Hardware queues"). */
#define AIC_MAX_IN_FLIGHT 32u
int aic_render_submit(aic_ctx *ctx, const aic_frame_desc *frame, void *out_device, uint32_t slot);
int aic_render_wait(aic_ctx *ctx, uint32_t slot, aic_frame_info *info);
/* Several frames in ONE launch (ABI 3): n_frames = 1, 2, 4 or 8 frames of the same size, partition, flags and tuning, each with its own cameras, backdrop
 * and output buffer (out_devices[i], device memory), under the scene and options as they stand -- the frames a recording loop knows ahead of time
 * (record.rs:97-113 steps a camera path over a scene that does not change), or a rank's shares of consecutive frames of a multi-GPU stream. The
 * persistent grid is split between the frames (every workgroup traces one of them, each frame has its own tile queues and cost record), so they are
 * resident side by side by construction: n small frames fill the chip like one large one -- one ramp, one tail, and the lane-exchanging variant where
 * a frame alone would be too small for it -- instead of n launches that share the hardware queues as the runtime sees fit. The batch occupies `slot`
 * like one frame: aic_render_wait reports the sums of its frames' counts, aic_render_wait_batch each frame's; aic_stream_wait_frame orders a foreign
 * stream behind all of them. Every frame's pixels and counts are those of the same frame submitted alone. */
int aic_render_submit_batch(aic_ctx *ctx, uint32_t n_frames, const aic_frame_desc *frames, void *const *out_devices, uint32_t slot);
int aic_render_wait_batch(aic_ctx *ctx, uint32_t slot, uint32_t n_frames, aic_frame_info *infos);
/* replaces: RtScene::trace_patch (renderer.rs:418-451) for a batch of pixel rectangles -- the call
 * all-is-cubes-gpu's raytrace_to_texture makes for its incremental pixel batches
 * (raytrace_to_texture.rs:603-633). rects = [n][4] {min.x, min.y, max.x, max.y} in normalized device
 * coordinates; each is traced like one image pixel (its centre, or the four antialiasing points).
 * out_rgba8 = [n] encoded pixels and aux (may be NULL) = [n] first-hit records, both host memory.
 * Only the cameras, backdrop and flags of `frame` are used. */
int aic_trace_patches(aic_ctx *ctx, const aic_frame_desc *frame, uint32_t n, const double *rects, void *out_rgba8,
                      aic_pixel_aux *aux, aic_frame_info *info);
/* replaces: SpaceRaytracer::trace_ray(ray, accumulator, include_sky) (sr.rs:113-120) for a batch of world-space rays against ONE layer's space:
 * no camera, no pixel grid -- picking rays that are not pixels, panoramic / fisheye / cube-map projections made by the host, light probes, line-of-sight
 * batches. rays = [n][6] {origin x, y, z, direction x, y, z}; each is traced as trace_ray_impl(ray, ColorBuf, include_sky, allow_ray_bounce = true) under
 * the layer's options and nothing of the image path: one ray per result whatever `antialiasing` says, no UI / world layering, no backdrop, no
 * "no world to show" paint. A direction is taken as given, not normalised (t runs in units of it); zero, NaN and infinite components are legal and
 * trace what the reference traces for them (no steps, the sky). LightingOption::Bounce seeds its generator from the direction's bits (sr.rs:165-178).
 * flags: AIC_FRAME_OUT_COLORBUF (out = [n] float[4], what trace_ray leaves in its accumulator) | AIC_FRAME_OUT_LINEAR (out = [n] float[4],
 * Rgba::from(ColorBuf)) | neither (out = [n] sRGB RGBA8 under the layer's tone mapping and `exposure`) | AIC_FRAME_COUNTERS | AIC_RAYS_NO_SKY |
 * AIC_RAYS_DEVICE; other AIC_FRAME_* bits are ignored. Bits 9-10 (AIC_TUNE_VARIANT_SHIFT) ask for a production variant of the trace kernel as
 * aic_frame_desc.tuning does (measurement and tests; 0: by the batch's size; any value gives the same results). aux (may be NULL) = [n] first-hit records, `layer` = the layer traced; info as for
 * aic_trace_patches (rows_rendered = n). The call returns when the batch is done. AIC_ERR_INVALID: a frame still occupies slot 0, a layer without a
 * space, more than 2048 x 65535 rays, a NaN or negative exposure, both float flags; AIC_ERR_UNSUPPORTED: AIC_FRAME_BLOOM. n = 0 is AIC_OK. */
#define AIC_RAYS_NO_SKY 128u /* include_sky = false: a ray that hits nothing ends transparent, and fog takes no sky light (sr.rs:145-161, 228-237) */
#define AIC_RAYS_DEVICE 256u /* rays, out and aux are device pointers on the context's device (no staging copy, no read-back); rays at a 16-byte
                              * boundary -- an allocation's start, or any whole number of rays into one */
int aic_trace_rays(aic_ctx *ctx, int layer, uint32_t n, const double *rays, uint32_t flags, float exposure, void *out, aic_pixel_aux *aux,
                   aic_frame_info *info);
/* replaces: one round of Inner::do_some_tracing (all-is-cubes-gpu/src/raytrace_to_texture.rs:591-751) -- RtScene::trace_patch on each listed pixel's
 * own rectangle and the store of its texels at that pixel's position. pixels[i] = y * frame->width + x names pixel (x, y) of `frame`, which is traced
 * exactly as aic_render traces it for the same `frame` (layers, UI pre-pass, backdrop, the four antialiasing samples, AIC_FRAME_PIXEL_CENTERS, the
 * frame's pixel edges): the same bits. The output kind follows frame->flags as in aic_render: RGBA8, AIC_FRAME_OUT_LINEAR, AIC_FRAME_OUT_COLORBUF or
 * AIC_FRAME_OUT_SPLIT. AIC_FRAME_COUNTERS is honoured; info->rows_rendered = n, info->variant = AIC_VARIANT_RECORDING (pixel lists always run the
 * recording variants, as Split frames do).
 * mode 0 (compact): out = [n] results in list order, host memory; for Split [n] colour texels, then [n] f32 depths at byte offset n * 8.
 * AIC_PIXELS_DEVICE: `pixels`, `out` and `aux` are device pointers on the context's device (no staging copy, no read-back).
 * AIC_PIXELS_IN_PLACE (needs AIC_PIXELS_DEVICE): out is a whole frame as aic_render with no partition lays it out (Split: the depth plane at byte
 * offset width * height * 8); result i goes to pixel pixels[i] and every other texel is left as it is -- the resident textures of raytrace_to_texture.
 * aux (may be NULL) = [n] first-hit records in list order, whatever the mode. A pixel may be listed more than once (PixelPicker's inner cycle
 * repeats pixels): every store of it carries the same value. The call returns when the batch is done (slot 0, like aic_trace_patches). n = 0 is AIC_OK.
 * AIC_ERR_INVALID: a frame still occupies slot 0; a host list with an entry >= width * height; more than 2048 x 65535 pixels; width or height above
 * 65535; AIC_PIXELS_IN_PLACE without AIC_PIXELS_DEVICE; AIC_FRAME_OUT_SPLIT with a float flag; a device `out` that is not at its element's boundary
 * (8 bytes for Split, 16 for the float outputs); a negative or NaN exposure. AIC_ERR_UNSUPPORTED: AIC_FRAME_BLOOM, partition.n_parts > 1. The
 * context stays usable after either. A device list cannot be checked by the host: an entry >= width * height gets no ray and no store and counts
 * nothing (its aux record is left as it is). */
#define AIC_PIXELS_DEVICE 1u   /* `pixels`, `out` and `aux` are device pointers on the context's device */
#define AIC_PIXELS_IN_PLACE 2u /* `out` is a whole frame of frame->width x frame->height; result i goes to pixel pixels[i], every other texel is left
                                * as it is. Needs AIC_PIXELS_DEVICE */
int aic_trace_pixels(aic_ctx *ctx, const aic_frame_desc *frame, uint32_t n, const uint32_t *pixels, uint32_t mode, void *out, aic_pixel_aux *aux,
                     aic_frame_info *info);
/* replaces: PixelPicker::new (raytrace_to_texture.rs:838-908), the order in which do_some_tracing takes a frame's pixels: centre first, dithered, the
 * central pixels interleaved with the rest. Host-only, like aic_light_chart. order (may be NULL) = [width * height]: the pixel indices y * width + x
 * stably sorted by (int64)(max(|x - cx|, |y - cy|) + ((x ^ y) % 4) * 2) evaluated in f64, c = size / 2 - 0.5. *central = min(60000, count / 4);
 * *cycle_length = 2 * max(central, count - central) (either may be NULL). The pick sequence, k = 0, 1, 2, ...: pick k is order[(k / 2) % central] for
 * even k and order[central + (k / 2) % (count - central)] for odd k; with central = 0 every pick k is order[k % count] (itertools::Interleave with one
 * side empty). The first cycle_length picks cover every pixel. An empty viewport gives AIC_OK, zeros, and nothing written. */
int aic_pixel_order(uint32_t width, uint32_t height, uint32_t *order, uint32_t *central, uint64_t *cycle_length);
/* replaces: the reprojection of raytrace_to_texture's resident textures into the current camera when it has moved since they were traced
 * (all-is-cubes-gpu/src/raytrace_to_texture.rs:433-540 prepare_frame; shaders/rt-copy.wgsl:73-223 rt_reproject_vertex / rt_reproject_fragment, drawn
 * with a LessEqual depth test, pipelines.rs:633-674), followed by the gap fill (shaders/resampling.wgsl:119-176 through mip_ping with 12 levels and
 * one repetition, raytrace_to_texture.rs:150-172 and 326-335). Every pixel of `src` becomes one depth-tested point sprite in the new view; the pixels no
 * sprite covers are filled from a nearest-sampled mip pyramid. DESIGN.md 4.10 restates every operation (all f32, one rounding each, in the order
 * written there) and the five decisions taken where the reference leaves room; tests/reproject_ref.py is that text in NumPy and the device equals it
 * bit for bit.
 * src_device, dst_device: whole Split frames of width x height as aic_render with no partition lays them out: the colour plane [height][width] of
 * four f16, then the depth plane [height][width] of f32 at byte offset width * height * 8 (sign bit set: a UI pixel). dst is again such a frame -- it
 * can be handed to aic_trace_pixels in place, or reprojected again: colour = the winning sprite's texel or the fill, alpha -1 where nothing is known
 * (the marker 0, 0, 0, -1); depth = the winning fragment's depth in the new view (sign bit: the winner was a UI pixel), 1.0 where no sprite landed.
 * The call blocks and runs on slot 0, like aic_trace_pixels. Scratch belongs to the context, is allocated on first use and again when a frame needs more:
 * the depth-test keys (8 bytes a pixel), the splat image (8 bytes a pixel), mips 1 .. L-1 of the chain (8 bytes a texel; mip 0 is never stored) and four
 * counters -- aic_reproject_geometry reports it; 1920 x 1080 (L = 11, T0 = 2048 x 2048): 33 177 600 + 11 184 800 + 32 = 44 362 432 bytes.
 * Rejected before anything is queued, with AIC_ERR_INVALID and the context still usable: a frame still occupying slot 0; a NULL pointer; src or dst not
 * at an 8-byte boundary; src and dst ranges that overlap (equal pointers included); width or height above 65535; a matrix or inverse_projection_zw
 * component that is not finite; unknown flag bits. A width or height of 0 is AIC_OK, writes nothing and zeroes the info. */
#define AIC_REPROJECT_KEEP_SPLATS 1u  /* a pixel some sprite covered with a valid texel keeps that texel at full resolution; without it (the reference's
                                       * behaviour) the last upsample returns mip 1 wherever that is valid, which halves the image's resolution */
#define AIC_REPROJECT_MAX_LEVELS 12u  /* raytrace_to_texture.rs:331 */
typedef struct aic_reproject_desc {
    uint32_t width, height;      /* size of BOTH frames (the reference reprojects at the render viewport's own size) */
    float reprojection[16];      /* ReprojectionUniforms.reprojection_matrix as WGSL holds it: column-major, [c*4+r];
                                    clip_new = M * clip_old (column vector) */
    float inverse_projection_zw[4]; /* {ipz.z, ipw.z, ipz.w, ipw.w} of the CURRENT camera's inverse projection
                                       (rt-copy.wgsl:210-223) */
    uint32_t flags;              /* AIC_REPROJECT_* */
    uint32_t reserved;
} aic_reproject_desc;
typedef struct aic_reproject_info {
    uint64_t n_splats;    /* source pixels that drew a sprite */
    uint64_t n_dropped;   /* source pixels that drew none (behind the camera, degenerate) */
    uint64_t n_gaps;      /* pixels no sprite covered, before the fill */
    uint64_t n_unfilled;  /* pixels of the result whose colour is still the invalid marker */
    float kernel_ms;      /* HIP events around the whole post-process */
    uint32_t levels;      /* L */
    uint32_t t0[2];       /* T0 */
} aic_reproject_info;
int aic_reproject_split(aic_ctx *ctx, const aic_reproject_desc *desc, const void *src_device, void *dst_device, aic_reproject_info *info);
/* host-only, like aic_pixel_order: levels L = min(12, ilog2(min(width, height)) + 1), T0 = (width, height) each rounded up to a multiple of 2^L, and
 * the bytes of context scratch the call needs (any of the three may be NULL). An empty viewport gives zeros. AIC_ERR_INVALID: width or height
 * above 65535. */
int aic_reproject_geometry(uint32_t width, uint32_t height, uint32_t *levels, uint32_t t0[2], uint64_t *scratch_bytes);
/* replaces: PixelPicker::take (all-is-cubes-gpu/src/raytrace_to_texture.rs:838-908) on the device -- the next n pixel indices written into device
 * memory, ready for aic_trace_pixels(..., AIC_PIXELS_DEVICE | AIC_PIXELS_IN_PLACE) -- and adds what the reference does not have: on request the list
 * begins with the pixels the context's last reprojection knows nothing about. Opt-in through max_unknown, as AIC_REPROJECT_KEEP_SPLATS is: with
 * max_unknown = 0 the list is exactly the pick sequence written out under aic_pixel_order. DESIGN.md 4.12; tests/pick_ref.py is that text in NumPy and
 * the device equals it entry for entry, on every run.
 * count = width * height. order_device = [count], the result of aic_pixel_order uploaded once by the caller; NULL: row-major, order[r] = r. It is
 * not checked: an entry >= count is never unknown, and in the picker part it is written as it is (aic_trace_pixels ignores such an entry of a device
 * list). Unknown set U: the pixels p whose texel of the splat image R that the context's last successful aic_reproject_split left in its scratch has
 * !(alpha > -0.5), the gap fill's validity test: no sprite covered p, the winning sprite carried the marker texel, or its alpha is NaN. Rank list
 * u_0, u_1, ...: the pixels order[r], r ascending, that are in U; n_unknown = |U|. g = min(n, max_unknown, max(n_unknown - skip_unknown, 0)).
 * pixels_out[i] = u_(skip_unknown + i) for i < g; pixels_out[g + j] = pick(cursor + j) for j < n - g, pick k being order[(k / 2) % central] for even
 * k and order[central + (k / 2) % (count - central)] for odd k, central = min(60000, count / 4); with central = 0, order[k % count]; all 64-bit.
 * Nothing beyond pixels_out[n) is written; R, the frames and the keys are only read. With max_unknown = 0 R is not looked at and n_unknown is 0.
 * The call blocks and runs on slot 0, like aic_reproject_split. Scratch of its own (8 bytes per 256 pixels and a 32-byte record) belongs to the
 * context, is allocated on first use with max_unknown > 0, again when a frame needs more, and released in aic_destroy.
 * Rejected before anything is queued, with AIC_ERR_INVALID and the context still usable: a NULL desc or info; a NULL pixels_out_device with n > 0;
 * pixels_out_device or order_device not at a 4-byte boundary; n > 0 with count = 0; width or height above 65535; n above 2048 x 65535
 * (aic_trace_pixels' limit); non-zero flags; a frame still occupying slot 0; max_unknown > 0 when the context's last successful aic_reproject_split
 * was not of exactly width x height (one of another size replaces that state; a failed, a rejected or an empty one leaves it as it was). n = 0 is AIC_OK,
 * writes nothing and zeroes the info. */
typedef struct aic_pick_desc {
    uint32_t width, height;  /* the resident frame */
    uint32_t n;              /* picks to write */
    uint32_t max_unknown;    /* at most this many of them from the unknown pixels of the last reprojection; 0: none */
    uint64_t skip_unknown;   /* unknown pixels (in rank order) already handed out since that reprojection */
    uint64_t cursor;         /* pick index k of the first picker pick */
    uint32_t flags;          /* none defined: must be 0 */
    uint32_t reserved;
} aic_pick_desc;
typedef struct aic_pick_info {
    uint64_t n_unknown;      /* unknown pixels of the last reprojection (0 when max_unknown == 0: not looked at) */
    uint64_t next_cursor;    /* cursor + n_from_order */
    uint32_t n_from_unknown; /* g */
    uint32_t n_from_order;   /* n - g */
    float kernel_ms;         /* HIP events around the launches */
    uint32_t reserved;
} aic_pick_info;
int aic_pick_pixels(aic_ctx *ctx, const aic_pick_desc *desc, const uint32_t *order_device, uint32_t *pixels_out_device, aic_pick_info *info);
/* Adds what the reference does not have: after a scene change (aic_update_cubes, aic_replace_blocks) under a resident Split frame, the next picks are
 * first the resident pixels the changed cubes can have changed, instead of a whole picker cycle re-armed by Inner::dirty()
 * (all-is-cubes-gpu/src/raytrace_to_texture.rs:587-589). Two entry points; DESIGN.md 4.17 states the rule, tests/stale_ref.py is that text in NumPy.
 *
 * aic_stale_rects (host-only, f64, like aic_exposure_rays and aic_cursor_wireframe) turns boxes of changed cubes into screen rectangles. A pixel's value
 * depends only on the cubes its sample rays pass through and, at a lit surface, on the cubes within one cube of the hit cube (the interpolated light
 * stencil, the light-leak fix, ambient occlusion), and every sample ray of pixel (x, y) passes through an NDC point inside that pixel's square; so under
 * an unchanged light volume a changed box [lo, hi) can only change a pixel whose square meets the bounding rectangle of the projected box grown by one
 * cube: expand = 1. view_projection: camera.projection * camera.view_matrix as aic_lines_desc holds it (column-major [c*4+r], clip = M (x, y, z, 1)),
 * in double. boxes = [n_boxes][6] {lo x, y, z, hi x, y, z}, upper bounds exclusive. Per box, in this order:
 *   - hi <= lo on some axis (no volume): the empty rectangle, all fields 0.
 *   - the eight corners of [lo - expand, hi + expand] (64-bit integers, then doubles) are projected, clip_r = ((M[r] x + M[4+r] y) + M[8+r] z) + M[12+r],
 *     one rounding each. If a corner's w is not > 0 or a clip coordinate is not finite: the whole frame {0, 0, width, height} and dmin = -inf (the camera
 *     inside or beside the box).
 *   - otherwise, with [ax, bx] x [ay, by] the bounds of the eight x / w, y / w: columns floor((ax + 1) / 2 * width) - 1 up to and including
 *     floor((bx + 1) / 2 * width) + 1, rows floor((1 - by) / 2 * height) - 1 up to and including floor((1 - ay) / 2 * height) + 1 (row 0 at NDC
 *     y = +1: Viewport::normalize_fb_x_edge / _y_edge inverted; the pixel on every side is there against rounding), clamped to the frame; if no column
 *     or no row is left, the empty rectangle, all fields 0.
 *   - dmin = the least z / w of the eight, less 2^-24, rounded DOWN to f32 (DESIGN.md 4.17 on the margin).
 * AIC_ERR_INVALID: a NULL pointer with n_boxes > 0, a negative expand, width or height above 65535, a matrix component that is not finite.
 *
 * aic_pick_stale is aic_pick_pixels with the unknown set U replaced by the stale set S of the resident frame `src_device` (a whole Split frame of
 * width x height as aic_render with no partition lays it out): the pixels inside at least one rectangle that does not keep them out. Without
 * AIC_STALE_DEPTH_TEST no rectangle keeps a pixel out: always conservative, and the frame is not read. With it rectangle b keeps pixel p out iff p's depth
 * texel has a clear sign bit, p's alpha half is >= 1 (so not NaN, not the marker) and depth < b.dmin in f32: UI pixels, pixels of no layer, -0.0,
 * translucent pixels, marker texels and NaN depths are always stale inside a rectangle. The flag needs a frame traced under the camera's own depth
 * transform (Camera::depth_transform_zw(), as aic_present_split_lines' depth test does) and is the caller's knowledge and opt-in, as
 * AIC_REPROJECT_KEEP_SPLATS is: it is exact only where no translucent surface lies in front of the changed cubes (a glass pane in front of an opaque
 * wall stores the PANE's depth, and the alpha of what lies behind it), and, in an antialiased frame, only for pixels whose four samples all end in front
 * of the box (the depth texel is the NEAREST sample's: a pixel on an occluder's silhouette is kept out although a sample passes the occluder).
 * Rank list s_0, s_1, ...: the pixels order[r], r ascending, that are in S (an entry >= count is never stale); n_stale = |S|.
 * g = min(n, max_stale, max(n_stale - skip_stale, 0)); pixels_out[i] = s_(skip_stale + i) for i < g; pixels_out[g + j] = pick(cursor + j) for
 * j < n - g, pick exactly as under aic_pick_pixels; all 64-bit. With n_rects = 0 or max_stale = 0 nothing is looked at, n_stale is 0 and the list is the
 * picker's. A pixel may appear both in the stale part and in the picker part: harmless, as with unknown pixels. Nothing beyond pixels_out[n) is written;
 * src is only read. The call blocks and runs on slot 0, like its siblings. rects is host memory, copied into context scratch before the call returns
 * (empty rectangles are left out of the copy). Scratch (40 bytes per 256 pixels, 16 a rectangle and a 32-byte record) belongs to the context, is allocated
 * on first use, again when a call needs more, and released in aic_destroy.
 * Rejected before anything is queued, with AIC_ERR_INVALID and the context still usable: everything aic_pick_pixels rejects for the arguments the two
 * share (a NULL desc or info; a NULL pixels_out_device with n > 0; pixels_out_device or order_device off a 4-byte boundary; n > 0 with count = 0; width
 * or height above 65535; n above 2048 x 65535; a frame still occupying slot 0); src_device off an 8-byte boundary, or NULL when it would be read (n > 0,
 * n_rects > 0, max_stale > 0 and the depth test); NULL rects with n_rects > 0; n_rects above AIC_STALE_MAX_RECTS (a caller with more boxes merges them
 * or passes one whole-frame rectangle); a rectangle with x0 > x1, y0 > y1, x1 > width or y1 > height; a NaN dmin; unknown flag bits. n = 0 is AIC_OK,
 * writes nothing and zeroes the info.
 * Limits: LightingOption::Bounce rays go anywhere. A light update changes cubes the caller did not edit, and more of them than AIC_STALE_MAX_RECTS:
 * aic_pick_stale_cubes below takes the changed light cubes themselves, any number of them. */
#define AIC_STALE_DEPTH_TEST 1u
#define AIC_STALE_MAX_RECTS 4096u
typedef struct aic_stale_rect {
    uint16_t x0, y0, x1, y1;  /* columns [x0, x1), rows [y0, y1) */
    float dmin;               /* nothing of the box is nearer than this depth; -inf: unknown */
    uint32_t reserved;
} aic_stale_rect;
typedef struct aic_stale_desc {
    uint32_t width, height;  /* the resident frame */
    uint32_t n;              /* picks to write */
    uint32_t max_stale;      /* at most this many of them from the stale pixels; 0: none */
    uint64_t skip_stale;     /* stale pixels (in rank order) already handed out under these rectangles */
    uint64_t cursor;         /* pick index k of the first picker pick */
    uint32_t n_rects;
    uint32_t flags;          /* AIC_STALE_* */
    const aic_stale_rect *rects;  /* host memory */
} aic_stale_desc;
typedef struct aic_stale_info {
    uint64_t n_stale;        /* |S| (0 when n_rects == 0 or max_stale == 0: not looked at) */
    uint64_t next_cursor;    /* cursor + n_from_order */
    uint32_t n_from_stale;   /* g */
    uint32_t n_from_order;   /* n - g */
    float kernel_ms;         /* HIP events around the launches */
    uint32_t reserved;
} aic_stale_info;
int aic_stale_rects(const double view_projection[16], uint32_t width, uint32_t height, uint32_t n_boxes, const int32_t *boxes /* [n][6] */, int32_t expand,
                    aic_stale_rect *out /* [n] */);
int aic_pick_stale(aic_ctx *ctx, const aic_stale_desc *desc, const void *src_device, const uint32_t *order_device, uint32_t *pixels_out_device,
                   aic_stale_info *info);
/* Adds what the reference does not have: aic_pick_stale for any number of changed boxes and changed LIGHT cubes, projected on the device, so that a light
 * update (hundreds to tens of thousands of changed texels) is complete in the next displayed frame too. The cost follows the rectangles' area and not
 * pixels x rectangles. DESIGN.md 4.19 states the rule; tests/stale_cubes_ref.py is that text in NumPy.
 *
 * The set. S = the pixels of the resident frame inside at least one rectangle that does not keep them out.
 *   - boxes[n_boxes][6] are changed BLOCKS: a box's rectangle is aic_stale_rects' own under view_projection, width, height and expand: x0, y0, x1, y1 and
 *     dmin bit for bit.
 *   - light_cubes[n_light_cubes][3] are cubes whose LIGHT texel changed with the blocks as they are. A pixel's value depends on light only at a lit
 *     surface, through the texels within one cube of the hit cube; so a changed texel at cube q can change only pixels with a surface inside
 *     [q - 1, q + 2): the rectangle of the box [q, q + 1) with expand = 1 (the desc's expand is not used), plus dmax = the greatest z / w of the eight
 *     corners, plus 2^-24, rounded UP to f32; dmax = +inf where dmin is -inf.
 *   - With AIC_STALE_DEPTH_TEST any rectangle keeps a pixel out as under aic_pick_stale: the depth texel's sign bit is clear, the alpha half is >= 1 and
 *     depth < dmin in f32. The caller's knowledge, with the three caveats stated there.
 *   - With AIC_STALE_DEPTH_BEHIND a LIGHT rectangle also keeps a pixel out iff the depth texel's sign bit is clear, the alpha half is > -0.5 (aic_pick_pixels'
 *     validity test: a NaN alpha and the marker texel, whose alpha is -1, stay stale) and depth > dmax in f32. This needs only a frame traced under the camera's own depth transform, and is exact under translucency
 *     and antialiasing: a Split frame's depth texel is the depth of the NEAREST surface of the pixel -- nearest over a ray's surfaces, glass included,
 *     and nearest over the four samples of an antialiased pixel --, so a depth beyond the grown box's greatest depth says that every surface of every
 *     sample lies behind the box, and the texel cannot matter. No opaque alpha is asked for. Boxes never use this test: a changed block in front of a
 *     surface can hide it.
 * The list is aic_pick_stale's: the ranks of order_device in S ascending; g = min(n, max_stale, max(n_stale - skip_stale, 0)); then the picker from
 * cursor; all 64-bit. With n_boxes + n_light_cubes = 0 or max_stale = 0 nothing is looked at, n_stale, n_rects and whole_frame are 0 and the list is the
 * picker's. There is no cap on the counts but that their sum fits 32 bits, and memory. boxes and light_cubes are host memory, copied into context
 * scratch before the call returns. A rectangle that is the whole frame with no depth bound the flags can use (the camera inside or beside the grown box)
 * makes every pixel stale at once: info.whole_frame is 1 and no rectangle is marked. Scratch (4 bytes per 32 pixels of a row, 40 bytes per 256 pixels,
 * 24 a rectangle, the arrays and a 32-byte record) belongs to the context, is allocated on first use, again when a call needs more, and released in
 * aic_destroy. The call blocks and runs on slot 0, like its siblings; src is only read, and only with a depth flag that some rectangle can use.
 * Rejected before anything is queued, with AIC_ERR_INVALID and the context still usable: everything aic_pick_stale rejects for the arguments the two
 * share (a NULL desc or info; a NULL pixels_out_device with n > 0; pixels_out_device or order_device off a 4-byte boundary; n > 0 with count = 0; width
 * or height above 65535; n above 2048 x 65535; a frame still occupying slot 0; src_device off an 8-byte boundary, or NULL when it would be read: n > 0,
 * max_stale > 0 and AIC_STALE_DEPTH_TEST with any box or cube, or AIC_STALE_DEPTH_BEHIND with a light cube; unknown flag bits); NULL boxes with
 * n_boxes > 0; NULL light_cubes with n_light_cubes > 0; n_boxes + n_light_cubes above 2^32 - 1; a negative expand; a component of view_projection that
 * is not finite. n = 0 is AIC_OK, writes nothing and zeroes the info.
 * aic_probe_stale_cube_rects copies the projected rectangles back to host memory: out[n_boxes + n_light_cubes], the boxes' first, all fields 0 for a
 * dropped one, dmax also for boxes (which never use it). It uses the desc's width, height, view_projection, expand and the two arrays, and rejects what
 * aic_pick_stale_cubes rejects of those.
 * Limits: LightingOption::Bounce rays go anywhere. */
#define AIC_STALE_DEPTH_BEHIND 2u
typedef struct aic_stale_cubes_desc {
    uint32_t width, height;  /* the resident frame */
    uint32_t n;              /* picks to write */
    uint32_t max_stale;      /* at most this many of them from the stale pixels; 0: none */
    uint64_t skip_stale;     /* stale pixels (in rank order) already handed out under these boxes and cubes */
    uint64_t cursor;         /* pick index k of the first picker pick */
    double view_projection[16];  /* as aic_stale_rects takes it */
    uint32_t n_boxes;
    int32_t expand;          /* the boxes are grown by this many cubes, as under aic_stale_rects */
    uint32_t n_light_cubes;
    uint32_t flags;          /* AIC_STALE_DEPTH_TEST | AIC_STALE_DEPTH_BEHIND */
    const int32_t *boxes;        /* [n_boxes][6] {lo x, y, z, hi x, y, z}, upper bounds exclusive; host memory */
    const int32_t *light_cubes;  /* [n_light_cubes][3]; host memory */
} aic_stale_cubes_desc;
typedef struct aic_stale_cubes_info {
    uint64_t n_stale;        /* |S| (0 when nothing was looked at) */
    uint64_t next_cursor;    /* cursor + n_from_order */
    uint32_t n_from_stale;   /* g */
    uint32_t n_from_order;   /* n - g */
    float kernel_ms;         /* HIP events around the launches */
    uint32_t reserved;
    uint32_t n_rects;        /* boxes and cubes whose rectangle holds a pixel */
    uint32_t whole_frame;    /* 1: a whole-frame rectangle without a usable depth bound made every pixel stale */
} aic_stale_cubes_info;
typedef struct aic_stale_cube_rect {
    uint32_t x0, y0, x1, y1; /* columns [x0, x1), rows [y0, y1) */
    float dmin;              /* nothing of the grown box is nearer than this depth; -inf: unknown */
    float dmax;              /* nothing of the grown box is farther than this depth; +inf: unknown */
} aic_stale_cube_rect;
int aic_pick_stale_cubes(aic_ctx *ctx, const aic_stale_cubes_desc *desc, const void *src_device, const uint32_t *order_device,
                         uint32_t *pixels_out_device, aic_stale_cubes_info *info);
int aic_probe_stale_cube_rects(aic_ctx *ctx, const aic_stale_cubes_desc *desc, aic_stale_cube_rect *out /* [n_boxes + n_light_cubes] */);
/* Adds what the reference does not have: the third kind of scene change under a resident frame, a block DEFINITION that changed (the reference's
 * todo.blocks, updating.rs:139-153; here aic_replace_block(s)). The cube grid does not change under such a call, only what the cubes holding that index
 * look like; aic_find_block_cubes finds those cubes in the layer's resident grid, and aic_pick_stale_blocks is aic_pick_stale_cubes with their boxes
 * added on the device. DESIGN.md 4.20 states the rule; tests/stale_blocks_ref.py is that text in NumPy.
 *
 * The rule. The layer's grid has size (sx, sy, sz) and lower corner lo; entry i = (x * sy + y) * sz + z (x, y, z from 0).
 *   - The index of an entry is its low 14 bits when the layer's grid carries tags (a block table of at most 16384 entries), else the entry itself. A cube
 *     the library has marked OPEN keeps its index bits and matches like any other.
 *   - match[i]: the entry's index is one of block_indices[n_blocks]. Duplicates among them are legal.
 *   - A run is a maximal stretch of consecutive matching entries inside one (x, y) row; runs never continue from z = sz - 1 into the next row.
 *   - The run list is sorted by the first entry's linear index. Box k is {lo.x + x, lo.y + y, lo.z + z0, lo.x + x + 1, lo.y + y + 1, lo.z + z1}, upper
 *     bounds exclusive, for the run z0 .. z1 - 1 of row (x, y).
 *   - info.n_cubes is the number of matches, info.n_runs the number of runs, info.bounds the smallest box holding all matches, all 0 when there are none.
 * What is written to out_boxes[capacity][6] (host memory):
 *     n_runs <= capacity                 every run, in order      n_written = n_runs   merged = 0
 *     n_runs > capacity, capacity >= 1   the one box `bounds`     n_written = 1        merged = 1
 *     n_runs > capacity, capacity = 0    nothing                  n_written = 0        merged = 1
 *     n_runs = 0                         nothing                  n_written = 0        merged = 0
 * so that a block filling half the world costs one box and not gigabytes of scratch. The result is the same bytes on every run.
 *
 * aic_pick_stale_blocks, by composition: the list and info.pick are exactly what aic_pick_stale_cubes gives for desc.cubes with, behind its own boxes,
 * the found.n_written boxes of aic_find_block_cubes(layer, block_indices, max_runs) -- same expand, flags, skip_stale, cursor and light cubes. The found
 * boxes never leave the device. With n_blocks = 0 the call is aic_pick_stale_cubes itself; when nothing is looked at (cubes.n = 0 or cubes.max_stale = 0)
 * no find runs and info.found is all 0. pick.kernel_ms covers the pick's launches and found.kernel_ms the find's.
 *
 * Both calls block, run on slot 0 and take its rule (no frame may occupy slot 0), like their siblings, and are ordered behind every earlier scene call
 * (aic_upload_space, aic_update_cubes, aic_replace_block(s), aic_compact) the way a frame submitted at that point would be. They only read the grid, which
 * the light updater never writes: they do NOT end a pending aic_evaluate_light_submit, and they are legal with frames in flight on other slots. Scratch
 * (8 KB of set, 12 bytes per 2048 grid entries, 24 bytes a run written) belongs to the context, is allocated on first use, again when a call needs
 * more, and released in aic_destroy.
 * Rejected before anything is queued, with AIC_ERR_INVALID and the context still usable: a NULL info; NULL block_indices with n_blocks > 0; an index at
 * or above the layer's block count; a layer that is not 0 or 1 or has no space; out_boxes NULL with capacity > 0; for aic_pick_stale_blocks also
 * everything aic_pick_stale_cubes rejects and cubes.n_boxes + max_runs + cubes.n_light_cubes above 2^32 - 1. One of those rules is wider here: what a
 * find gives is known only once it has run, so with n > 0, max_stale > 0, n_blocks > 0 and a grid that is not empty a NULL src_device is rejected under
 * AIC_STALE_DEPTH_TEST, and under AIC_STALE_DEPTH_BEHIND when cubes.n_light_cubes > 0 (the behind test is a light cube's alone), also when the find
 * would give no box.
 * Limits: LightingOption::Bounce rays go anywhere. A found box is projected like any other box: one with a corner at or behind the camera plane once it
 * is grown by expand -- a cube holding the block beside or behind the camera, as happens whenever the camera stands inside the space among such cubes --
 * has the whole frame for its rectangle, and then every pixel is stale as before (info.pick.whole_frame = 1). The light the re-evaluated block gives off or blocks is the light updater's matter
 * (aic_light_cubes_changed, aic_light_changed_take), not found here. */
typedef struct aic_block_cubes_info {
    uint64_t n_cubes, n_runs;
    int32_t  bounds[6];      /* {lo x, y, z, hi x, y, z}, upper bounds exclusive */
    uint32_t n_written;      /* boxes written to out */
    uint32_t merged;         /* 1: n_runs > capacity, the runs were not written one by one */
    float    kernel_ms;      /* HIP events around the find's launches */
    uint32_t reserved;
} aic_block_cubes_info;
int aic_find_block_cubes(aic_ctx *ctx, int layer, uint32_t n_blocks, const uint32_t *block_indices /* host */, uint32_t capacity,
                         int32_t *out_boxes /* [capacity][6], host; may be NULL when capacity = 0 */, aic_block_cubes_info *info);
typedef struct aic_stale_blocks_desc {
    aic_stale_cubes_desc cubes;     /* everything aic_pick_stale_cubes takes */
    int32_t  layer;
    uint32_t n_blocks;
    const uint32_t *block_indices;  /* [n_blocks]; host memory */
    uint32_t max_runs;              /* capacity of the find */
    uint32_t reserved;
} aic_stale_blocks_desc;
typedef struct aic_stale_blocks_info {
    aic_stale_cubes_info pick;
    aic_block_cubes_info found;
} aic_stale_blocks_info;
int aic_pick_stale_blocks(aic_ctx *ctx, const aic_stale_blocks_desc *desc, const void *src_device, const uint32_t *order_device,
                          uint32_t *pixels_out_device, aic_stale_blocks_info *info);
/* Adds what the reference does not have: a cube grid that was MADE on the device -- by a cellular automaton, a falling-sand or fluid step, a model that
 * emits voxels, any torch code -- becomes the layer's scene without a trip through the host, and the call says which cubes changed, which is what
 * aic_pick_stale_cubes and aic_light_cubes_changed want to know. DESIGN.md 4.23 states the rule and the passes; tests/grid_replace_ref.py is that text in
 * NumPy.
 *
 * aic_replace_cube_grid. The layer's bounds, block table, voxel pool, palette and sky stay. The block index of every cube is replaced by
 * block_index_device[n_cubes]: plain indices in device memory on the context's device, entry (x * sy + y) * sz + z as in aic_upload_space. With
 * light_device ([n_cubes][4], PackedLight texels) the light volume is replaced too; NULL leaves it as it is.
 *   - Afterwards the grid holds, byte for byte, what aic_upload_space of the same space with that block_index leaves there: with a block table of at most
 *     16384 entries index | (class + 1) << 14, and 0 in the tag of an OPEN cube (aic_probe_cube_grid); past 16384 blocks plain indices.
 *     Nothing at or past entry n_cubes of the pool is written: the voxel volumes start there.
 *   - The change report is aic_find_block_cubes' rule and info with another match: match[i] = the new index differs from the index the entry held (the low
 *     14 bits of a tagged entry: tags and OPEN never count as change). Runs, their order, the boxes (upper bounds exclusive, straight into
 *     aic_stale_cubes_desc.boxes), n_cubes, n_runs, bounds, n_written and merged follow that call's table; everything is 0 when nothing changed.
 *     kernel_ms: HIP events around the call's launches.
 *   - The call blocks. Like aic_update_cubes it first waits for every frame in flight and ends a pending aic_evaluate_light_submit; it bumps the layer's
 *     version, so the light updater reads the new grid before its next step. Texels the caller replaced are the caller's own and are never reported by
 *     aic_light_changed_*. The caller's arrays must be complete before the call -- its stream synchronised, or ordered with aic_wait_event -- and are
 *     free again when it returns.
 * Rejected with AIC_ERR_INVALID, with grid, light and context untouched and usable: an index at or above the layer's block count anywhere in the array
 * (the count pass finds the largest before anything is written); a NULL info or array; a layer that is not 0 or 1 or has no space; an array that does not
 * start at a 16-byte boundary (light_device: 4-byte); out_boxes NULL with capacity > 0. An empty grid is AIC_OK with a zero info.
 *
 * aic_copy_cube_grid. out_device[n_cubes] = the layer's grid as plain indices, tags stripped; light_out_device[n_cubes][4] = the published light volume
 * as it stands. Either may be NULL. How a device simulation starts from an uploaded scene. It only reads: legal with frames in flight on other slots,
 * like aic_find_block_cubes, whose slot rule it takes (no frame may occupy slot 0); a pending aic_evaluate_light_submit is published first when the light
 * is asked for. out_device starts at a 16-byte boundary, light_out_device at a 4-byte one. Blocks.
 *
 * aic_update_light_volume_device. aic_update_light_volume with the source in device memory (4-byte aligned, on the context's device): double-buffered
 * into a spare volume, on the upload stream, behind a finished light job; frames in flight are not waited for. Blocks until the copy is done.
 *
 * Scratch (16 bytes per 2048 grid entries, 24 bytes a run written) belongs to the context, is allocated on first use, again when a call needs
 * more, and released in aic_destroy. */
int aic_replace_cube_grid(aic_ctx *ctx, int layer, const uint16_t *block_index_device /* [n_cubes], Z-major, plain indices */,
                          const uint8_t *light_device /* [n_cubes][4] or NULL */, uint32_t capacity,
                          int32_t *out_boxes /* [capacity][6], host; NULL iff capacity = 0 */, aic_block_cubes_info *info);
int aic_copy_cube_grid(aic_ctx *ctx, int layer, uint16_t *out_device /* [n_cubes] or NULL */, uint8_t *light_out_device /* [n_cubes][4] or NULL */);
int aic_update_light_volume_device(aic_ctx *ctx, int layer, const uint8_t *light_device);
/* replaces: what raytrace_to_texture does with its resident textures every displayed frame: RaytraceToTexture::draw
 * (all-is-cubes-gpu/src/raytrace_to_texture.rs:546-568) draws rt_frame_copy_vertex / rt_frame_copy_fragment (shaders/rt-copy.wgsl:41-71) into the linear
 * scene texture -- the pipeline's linear ClampToEdge sampler stretches the frame to the viewport (the reference traces at half the nominal size,
 * raytracer_size_policy, raytrace_to_texture.rs:985-990), alpha is discarded and 1.0 written --; bloom.rs:41-60 and mip_ping.rs:301-420 run the
 * dual-filter chain on that texture; postprocess_fragment (shaders/postprocess.wgsl:140-158, 251-276) mixes mix(scene, bloom, bloom_intensity), tone-maps
 * and converts to the output colour space. DESIGN.md 4.11 restates every operation (all f32, one rounding each, in the order written there) and the
 * decisions taken; tests/present_ref.py is that text in NumPy.
 * src_device: a whole Split frame of src_width x src_height in device memory as aic_render with no partition lays it out (AIC_FRAME_OUT_SPLIT). Only the
 * three colour halves of each texel are used: a colour above 65504 (Split stores overflow as infinity) reads as 65504; source alpha and the whole depth
 * plane have no influence, so the marker texel (0, 0, 0, -1) of an unfilled reprojection shows black. A NaN colour gives whatever the arithmetic gives.
 * out: [out_height][out_width] RGBA8 (4 bytes a pixel), or four f16 (8 bytes) with AIC_PRESENT_OUT_F16; as in aic_render a device pointer when
 * out_is_device != 0, host memory the call reads back into otherwise. The output may equal, exceed or fall below the source in either axis; at equal
 * size the scene texel is the source texel itself.
 * The call blocks and runs on slot 0, like aic_reproject_split. Scratch belongs to the context, is allocated on first use, again when a call needs
 * more, and released in aic_destroy: aic_present_geometry reports it.
 * Rejected before anything is queued, with AIC_ERR_INVALID and the context still usable: a frame still occupying slot 0; a NULL pointer; src not at an
 * 8-byte boundary; a device out not at its element's boundary (4 bytes for RGBA8, 8 for f16); a device out overlapping the src_width * src_height * 12
 * bytes of src; any dimension above 65535; an output of more than AIC_PRESENT_MAX_PIXELS pixels (the kernels' texel indices are 32-bit); src of zero
 * size with a non-empty output; bloom_intensity NaN, negative or infinite; maximum_intensity NaN or negative; tone_mapping other than 0 or 1; unknown
 * flag bits. An empty output (out_width or out_height 0) is AIC_OK, writes nothing and zeroes the info. */
#define AIC_PRESENT_OUT_F16 1u   /* out = [out_height][out_width] of four f16: the mixed, tone-mapped LINEAR colour and alpha 1.0 (the reference's
                                  * color_space_id 0 on an Rgba16Float surface, postprocess.wgsl:251-276), saturated at 65504; default: sRGB RGBA8 as
                                  * aic_render writes it, alpha byte 255 */
#define AIC_PRESENT_MAX_PIXELS 2147483648ull  /* out_width * out_height at most 2^31 */
typedef struct aic_present_desc {
    uint32_t src_width, src_height;   /* the resident Split frame (no partition; layout as AIC_FRAME_OUT_SPLIT) */
    uint32_t out_width, out_height;   /* the window's framebuffer; may equal, exceed or fall below the source (rt-copy.wgsl:41-71) */
    float bloom_intensity;            /* GraphicsOptions::bloom_intensity (postprocess.wgsl:140-158); 0 skips the chain */
    int32_t tone_mapping;             /* 0 Clamp, 1 Reinhard (graphics_options.rs:352-368) */
    float maximum_intensity;          /* may be +inf: no tone mapping */
    uint32_t flags;                   /* AIC_PRESENT_* */
} aic_present_desc;
typedef struct aic_present_info {
    float kernel_ms;      /* HIP events around the whole post-process */
    uint32_t levels;      /* L of the bloom chain on the output size (bloom.rs:41-60, mip_ping.rs:460-481) */
    uint32_t t0[2];       /* T0 */
    uint32_t bloomed;     /* 1: the chain ran (bloom_intensity > 0) */
    uint32_t reserved[3];
} aic_present_info;
int aic_present_split(aic_ctx *ctx, const aic_present_desc *desc, const void *src_device, void *out, int out_is_device, aic_present_info *info);
/* host-only, like aic_reproject_geometry: levels L and T0 of the bloom chain on the OUTPUT size (mip_ping.rs:460-481 on bloom.rs:50-53's half-size
 * request: R = ceil(out / 2), L = min(6, ilog2(min(R)) + 1), T0 = R rounded up to a multiple of 2^L), and the bytes of context scratch a call with
 * bloom_intensity > 0 allocates: the chain's mips (8 bytes a texel) and, when the output size differs from the source's, the scene texture (8 bytes an
 * output pixel); 1920 x 1080 from 1920 x 1080: 5 896 800; from 960 x 540: 22 485 600. bloom_intensity is known only at call time: a call with 0 needs and
 * allocates none of it. Not counted: the staging of a host-target call, which is the context's output buffer that aic_render uses. Any of the three may
 * be NULL. An empty output gives zeros. AIC_ERR_INVALID: a dimension above 65535, more than AIC_PRESENT_MAX_PIXELS output pixels, src of zero size
 * with a non-empty output. */
int aic_present_geometry(uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, uint32_t *levels, uint32_t t0[2], uint64_t *scratch_bytes);
/* replaces: the lines pass of EverythingRenderer::draw_frame_linear (all-is-cubes-gpu/src/everything.rs:616-658): after the traced frame is drawn into
 * the scene texture with its depth as frag_depth (shaders/rt-copy.wgsl:55-71) and before bloom and tone mapping, the line list -- the cursor's wireframe
 * and debug lines -- is drawn with lines_vertex / lines_fragment (shaders/blocks-and-lines.wgsl:902-919) by a LineList pipeline with
 * CompareFunction::Less, depth write and no blend (pipelines.rs:453-487). aic_present_split_lines is aic_present_split with that pass: the lines are
 * drawn into the scene texture S on the device, depth-tested against the resident Split frame's depth plane, and bloom and composite run on the result.
 * WebGPU leaves line rasterisation to the implementation; the rule here is DESIGN.md 4.13's (clip coordinates, Liang-Barsky clipping, one fragment per
 * major-axis pixel centre in [p0, p1), nearest depth texel, least depth wins and among equal depths the lowest line), tests/present_lines_ref.py is that
 * text in NumPy and the device equals it bit for bit. A fragment passes iff its depth texel has a clear sign bit, is not NaN and f < min(texel, 1):
 * the negative depth of a UI pixel or of a pixel of no layer hides every line, as frag_depth clamped to 0 does in the reference. Colours are linear RGBA
 * interpolated in screen space and written as f16 with alpha 1; nothing is written to src.
 * lines == NULL or n_lines == 0: the call is aic_present_split itself -- the same launches, no extra scratch, lines_info zeroed.
 * vertices: host memory, copied into context scratch before the call returns, or with AIC_LINES_DEVICE a device pointer. Their contents are not
 * checked: a line with a non-finite position or r, g, b component is dropped and counted in n_clipped_away; alpha is never read, whatever it holds.
 * The line scratch is the context's own: the 64-bit key image and the stored scene (8 bytes an output pixel each), a 32-byte record and the staged
 * vertices of a host list; allocated on first use, again when a call needs more, released in aic_destroy. aic_present_lines_scratch reports it.
 * Rejected like aic_present_split, and also: NULL vertices with n_lines > 0; n_lines above AIC_LINES_MAX; a device vertices pointer off a 4-byte
 * boundary; unknown flag bits; a non-finite component of view_projection. All AIC_ERR_INVALID, before anything is queued, the context still usable. */
typedef struct aic_line_vertex {
    float position[3];  /* world space */
    float color[4];     /* linear RGBA (WgpuLinesVertex, all-is-cubes-gpu/src/in_wgpu/vertex.rs:386-410); alpha is not used: no blend */
} aic_line_vertex;
#define AIC_LINES_DEVICE 1u      /* `vertices` is a device pointer on the context's device (4-byte aligned) */
#define AIC_LINES_MAX 1048576u   /* lines per call */
typedef struct aic_lines_desc {
    float view_projection[16];   /* camera.projection * camera.view_matrix as WGSL holds it: column-major [c*4+r]; clip = M * (x, y, z, 1) */
    uint32_t n_lines;            /* line i = vertices[2i], vertices[2i+1] (LineList) */
    uint32_t flags;              /* AIC_LINES_* */
    const aic_line_vertex *vertices;
} aic_lines_desc;
typedef struct aic_lines_info {
    uint64_t n_clipped_away;     /* lines that produced no segment: a non-finite position, r, g, b or clip coordinate, clipped away whole, w <= 0 at a clipped end */
    uint64_t n_fragments;        /* fragments generated inside the window */
    uint64_t n_passed;           /* ... that passed the depth test against the frame */
    uint64_t n_pixels;           /* output pixels that show a line */
} aic_lines_info;
int aic_present_split_lines(aic_ctx *ctx, const aic_present_desc *desc, const aic_lines_desc *lines, const void *src_device, void *out, int out_is_device,
                            aic_present_info *info, aic_lines_info *lines_info);
/* host-only, like aic_present_geometry: the bytes of line scratch a call with n_lines > 0 host vertices allocates, on top of what aic_present_geometry
 * reports (of which such a call never needs the stored scene: it keeps its own). A device list needs n_lines * 56 fewer. 1920 x 1080 with the cursor's
 * 28 lines: 33 179 200. AIC_ERR_INVALID as aic_present_geometry, or n_lines above AIC_LINES_MAX. n_lines = 0 or an empty output gives 0. */
int aic_present_lines_scratch(uint32_t src_w, uint32_t src_h, uint32_t out_w, uint32_t out_h, uint32_t n_lines, uint64_t *bytes);
/* replaces: impl Wireframe for Cursor (all-is-cubes/src/character/cursor.rs:219-278), host-only, in f64 and in the reference's order: the 12 edges of
 * the hit block's voxel bounds (scaled by 1 / resolution, translated to the cube, expanded by 0.001 * distance_to_point) in Aab::wireframe_points' order
 * (all-is-cubes-base/src/math/aab.rs:569-588); if face_selected is a real face, the 12 edges of that box shrunk by 1/128 and flattened onto the face;
 * if face_entered is a real face, the 4-line diamond with tips at 1/32 around point_entered + face * offset. 12, 16, 24 or 28 lines; positions as f32,
 * colour palette::CURSOR_OUTLINE = linear (0, 0, 0, 1). aic_cursor_raycast (below) makes the Cursor: its record begins with this struct.
 * AIC_ERR_INVALID: a NULL pointer, a face outside 0..6, resolution < 1, a negative voxel_size. */
typedef struct aic_cursor_desc {
    int32_t cube[3];
    int32_t face_entered, face_selected;   /* Face7 discriminants, as aic_pixel_aux.face */
    double point_entered[3];
    double distance_to_point;
    int32_t voxel_lo[3], voxel_size[3];    /* EvaluatedBlock::voxels_bounds() */
    int32_t resolution;
    int32_t reserved;
} aic_cursor_desc;
#define AIC_CURSOR_MAX_LINES 28u
int aic_cursor_wireframe(const aic_cursor_desc *cursor, aic_line_vertex *out /* [2 * 28] */, uint32_t *n_lines);
/* replaces: cursor_raycast (all-is-cubes/src/character/cursor.rs:26-107) for n rays against the layer's space as last updated; DESIGN.md 4.18,
 * tests/cursor_ref.py is this text in Python. Ray i = {origin, direction}; the direction is normalised first, d / sqrt(dx * dx + dy * dy + dz * dz) in
 * f64 with one rounding per operation. Then, for each step of Raycaster(origin, d).within(space bounds, false): a step whose t_distance is greater
 * than maximum_distance ends the ray with no Cursor; a block that is unselectable (AIC_BLOCK_UNSELECTABLE, AIC_BLOCK_AIR) is passed over; a
 * single-voxel block (AIC_BLOCK_ONE or resolution 1) is hit if its voxel is selectable, with face_selected = the step's face; in any other block the
 * sub-ray of RaycastStep::recursive_raycast (raycast.rs:458-476: origin (origin - cube) * resolution, the same direction, within the block's voxel
 * bounds with the exit step) is walked: face_selected is the face of its first step, whatever lies there (Within for a ray that starts inside the voxel
 * bounds), and the first selectable voxel is the hit; a block without one, or one whose voxel bounds the sub-ray misses, is passed over. Voxel
 * selectability: see AIC_BLOCK_VOXEL_SELECTABLE. A ray takes at most size_x + size_y + size_z + 3 steps, which no ray within the bounds exceeds.
 * One record per ray, 144 bytes. A miss (the reference's None) is all zero. A hit has hit = 1 and
 *   cursor: cube, face_entered = the step's face, face_selected, point_entered = step.intersection_point(ray), distance_to_point = t_distance if it is
 *       greater than 0, else 0 (PositiveSign::new_clamped), and the hit block's voxel bounds and resolution (0,0,0 / 1,1,1 / 1 for a single-voxel block):
 *       aic_cursor_wireframe takes it as it stands;
 *   block_index of the hit cube; voxel = the selectable voxel found, in block coordinates (0,0,0 for a single-voxel block);
 *   has_preceding = face_entered is not Within, and then preceding_cube = cube + the face's normal with preceding_block_index = its block index, or
 *       0xFFFFFFFF for a cube outside the bounds, where the reference reads AIR;
 *   light_hit, light_preceding: Space::get_light of the two cubes as texels r, g, b, status from the layer's current light volume; for a cube outside
 *       the bounds BlockSky::light_outside (sky.rs:113-147);
 *   steps: the steps of the outer Raycaster examined, the hit's included.
 * Zero, NaN and infinite components are legal and give what the reference's arithmetic gives up to where it would panic: no hit has a NaN distance.
 * flags: AIC_RAYS_DEVICE or 0 -- `rays` and `out` are device pointers at 8-byte boundaries, nothing is staged or read back. The call returns when the
 * records are there. Like aic_sample_luminance it is legal while frames are in flight and disturbs none of them, finishes a pending
 * aic_evaluate_light_submit first and sees every scene and light write issued before it. AIC_ERR_INVALID, the context still usable: a NULL pointer with
 * n > 0, a layer without a space, n above 1 << 20, unknown flag bits, a NaN or negative maximum_distance (+infinity is legal), misaligned device
 * pointers. n == 0 is AIC_OK. An aic_multi replicates the scene: a host of one raycasts through the context of its first device. */
typedef struct aic_cursor_hit {
    aic_cursor_desc cursor;
    int32_t hit;
    uint32_t block_index;
    int32_t voxel[3];
    int32_t has_preceding;
    int32_t preceding_cube[3];
    uint32_t preceding_block_index;
    uint8_t light_hit[4];
    uint8_t light_preceding[4];
    uint32_t steps;
    uint32_t reserved_hit;
} aic_cursor_hit;
#define AIC_CURSOR_NO_BLOCK 0xFFFFFFFFu /* preceding_block_index of a cube outside the bounds */
int aic_cursor_raycast(aic_ctx *ctx, int layer, uint32_t n, const double *rays /* [n][6] origin, direction */, double maximum_distance,
                       uint32_t flags /* 0 or AIC_RAYS_DEVICE */, aic_cursor_hit *out /* [n] */);
/* The info text -- the frame-rate and statistics overlay, on by default (GraphicsOptions::debug_info_text) -- of the interactive renderer, which is
 * part of its presentation's last shader: four entry points, DESIGN.md 4.14, tests/present_text_ref.py is that text in NumPy.
 *
 * aic_set_text_font replaces: the font atlas texture that generate_texture_atlas makes (all-is-cubes-gpu/src/text.rs:108-155) and
 * EverythingRenderer::new binds with its metrics (everything.rs:305-311). atlas_rgba8: host memory, a grid of 16 x 16 cells of cell_width x cell_height
 * RGBA8 texels with premultiplied alpha, [16 * cell_height][16 * cell_width][4], the cell of character code k at column k % 16, row k / 16;
 * cell_margin texels on every side of a cell lie outside the logical cell (room for an outline that overlaps the neighbouring cells). The library
 * knows no font, as the reference's shader knows none: the caller draws the atlas (the host mirror's info_text_font_atlas, the Rust shim's
 * font_atlas). The atlas is copied into device memory the context owns, and is resident until it is replaced or the context destroyed; a NULL atlas
 * drops it (the cell arguments are then not looked at). The call waits for nothing in flight, except that it is rejected while a frame occupies
 * slot 0. AIC_ERR_INVALID: a cell dimension outside 1..1024; 2 * cell_margin >= min(cell_width, cell_height). */
int aic_set_text_font(aic_ctx *ctx, const uint8_t *atlas_rgba8, uint32_t cell_width, uint32_t cell_height, uint32_t cell_margin);
/* replaces: character_texture_size (all-is-cubes-gpu/src/text.rs:20-52) and the two text fields of PostprocessUniforms::new (postprocess.rs:316-331),
 * host-only, in the reference's types and order: the logical cell is the cell less 2 * cell_margin; cols = max(1, (u32)ceil(nominal_width /
 * logical_width)) in f64, rows likewise; scale = (f32)nominal / (f32)(cols * logical) as an f32 division; origin = (f32)(origin_px / nominal) with an
 * f64 division (the reference passes (5, 5)). Any output may be NULL. AIC_ERR_INVALID: a nominal size that is not finite or <= 0; a cell or margin
 * aic_set_text_font rejects; cols or rows above 65535. */
int aic_text_geometry(double nominal_width, double nominal_height, uint32_t cell_width, uint32_t cell_height, uint32_t cell_margin, const double origin_px[2],
                      uint32_t *cols, uint32_t *rows, float scale[2], float origin[2]);
/* replaces: render_text_to_character_texture (all-is-cubes-gpu/src/text.rs:56-73), host-only: codes[rows][cols] is cleared to 0; '\n' starts a new
 * row; every other scalar value of the `len` bytes of UTF-8 is its code if <= 0xFF, else '?'; the column advances with saturation; a character outside
 * the grid is dropped (draw_to_texture.rs:69-81). Malformed UTF-8 decodes to U+FFFD, which becomes '?'. used, which may be NULL: the extent in columns
 * and rows of the non-zero cells (the reference's `nonzero` rectangle from the grid's origin). AIC_ERR_INVALID: NULL codes, NULL utf8 with len > 0,
 * cols or rows of 0 or above 65535. */
int aic_text_layout(const char *utf8, uint64_t len, uint32_t cols, uint32_t rows, uint8_t *codes /* [rows][cols] */, uint32_t used[2]);
/* replaces: render_text / render_character_cell and the text blend of postprocess_fragment (all-is-cubes-gpu/src/shaders/postprocess.wgsl:160-276),
 * with the character texture of everything.rs:777-806: aic_present_split_lines with the info text laid over the tone-mapped scene on the device, before
 * the output encoding. Per output pixel the four nearest cells of the code grid are looked up in the resident font atlas, the component-wise maximum
 * of their texels is the text, and x = tone_mapped * (1 - text.a) + text: the text is neither tone-mapped nor bloomed, and lies over any lines. Output
 * alpha stays 255 / 1.0. DESIGN.md 4.14 restates every operation (f32, one rounding each) and the device equals tests/present_text_ref.py bit for bit.
 * text == NULL: the call is aic_present_split_lines itself -- the same launches, the same scratch.
 * codes: [rows][cols] character codes (0 reads as a space), host memory staged into context scratch before the call returns, or with AIC_TEXT_DEVICE
 * a device pointer. scale, origin: aic_text_geometry's. The staging belongs to the context, is allocated on first use and released in aic_destroy.
 * Pixels that cannot show text pay next to nothing: when the atlas's cell 0x20 was all zero at aic_set_text_font, only the pixels within one cell of
 * the non-zero codes of a host list (of the whole grid for a device list) look anything up. This changes no bit of the image.
 * Rejected like aic_present_split_lines, and also: text given but no font set; NULL codes; cols or rows of 0 or above 65535; a non-finite component of
 * scale or origin; unknown flag bits. All AIC_ERR_INVALID, before anything is queued, the context still usable. */
#define AIC_TEXT_DEVICE 1u       /* `codes` is a device pointer on the context's device */
typedef struct aic_text_desc {
    float scale[2], origin[2];   /* info_text_coordinate_scale and info_text_origin (postprocess.rs:316-331): tc = (uv - origin) * scale */
    uint32_t cols, rows, flags;  /* the character texture's size; AIC_TEXT_* */
    const uint8_t *codes;
} aic_text_desc;
int aic_present_split_text(aic_ctx *ctx, const aic_present_desc *desc, const aic_lines_desc *lines /* may be NULL */, const aic_text_desc *text /* may be NULL */,
                           const void *src_device, void *out, int out_is_device, aic_present_info *info, aic_lines_info *lines_info);
/* replaces: RerunImageExport::start_frame_copy / perform_image_copy (all-is-cubes-gpu/src/rerun_image.rs:62-225) with rerun_frame_copy_color_fragment and
 * rerun_frame_copy_depth_fragment (shaders/rerun-copy.wgsl:47-88): the RGB-D export of the resident textures -- the scene colour resampled to a logging
 * size as sRGB8, and the depth buffer unprojected to a distance along the view axis, an f32 per pixel in the world's units, 0 where nothing was hit.
 * The intrinsics and pose that travel with the two planes (convert_camera_to_pinhole, rerun_image.rs:314-338) are host arithmetic on the camera: the
 * host mirror's Camera::pinhole and the Rust shim's caller have them. DESIGN.md 4.15 restates every operation in the order written here;
 * tests/export_ref.py is that text in NumPy and the device equals it bit for bit.
 * Colour: output pixel (x, y) holds exactly the bytes aic_present_split writes for the same src and sizes with bloom_intensity 0, tone_mapping 0,
 * maximum_intensity +inf and flags 0. The scene texel S is the source texel itself at equal size, else the ClampToEdge bilinear read at the pixel's
 * centre rounded to f16, colour saturated at 65504 either way; S is clamped and encoded by the exact sRGB8 encoder of aic_render, alpha byte 255 (what
 * the Rgba8UnormSrgb target of rerun_frame_copy_color_fragment does to scene_for_postprocessing_input). Decision: the reference resamples twice, frame ->
 * window -> logged size; this call resamples once, from the frame. The two agree when the window has the frame's size.
 * Depth: the nearest texel, never interpolated (rerun-copy.wgsl:73-88). u = (x + 0.5f) / out_width, v = (y + 0.5f) / out_height in f32;
 * ix = min((uint32)(u * (float)src_width), src_width - 1), iy likewise; d the depth texel at (ix, iy), c the colour texel there. The value is, in this
 * order: 0 if d has its sign bit set (a UI pixel, a pixel of no layer, -0.0) or is NaN; 0 if c is the "nothing known" marker of an unfilled reprojection
 * (its alpha half is not above -0.5); 0 if d == 1.0f (linearize_depth_value, rerun-copy.wgsl:47-51); else -(d * a + b) / (d * c + e) with {a, b, c, e} =
 * inverse_projection_zw, f32 with one rounding per operation -- aic_reproject_split's own linearisation. The first two rules are this library's: the
 * reference's depth attachment would clamp a negative texel to 0 and log a point on the near plane for every UI pixel.
 * info: n_surface counts the output pixels whose exported depth is finite and > 0, depth_min and depth_max are taken over them (0, 0 when there are
 * none); computed on the device whether or not depth_out is NULL.
 * color_out, depth_out: either may be NULL and is then not written; as in aic_render device pointers when out_is_device != 0, host memory the call
 * reads back into otherwise (staged through the context's output buffer, 4 bytes a pixel and plane). Nothing is written to src.
 * The call blocks and runs on slot 0, like aic_present_split. Its 8 KiB of counters belong to the context and are released in aic_destroy.
 * Rejected before anything is queued or allocated, with AIC_ERR_INVALID and the context still usable: a frame still occupying slot 0; a NULL desc or
 * src; color_out, depth_out and info all NULL; src not at an 8-byte boundary; a device color_out or depth_out not at a 4-byte boundary; a device
 * output overlapping the src_width * src_height * 12 bytes of src, or the other output; any dimension above 65535; an output of more than
 * AIC_PRESENT_MAX_PIXELS pixels; src of zero size with a non-empty output; a non-finite component of inverse_projection_zw; unknown flag bits. An empty
 * output (out_width or out_height 0) is AIC_OK, writes nothing and zeroes the info. */
typedef struct aic_export_desc {
    uint32_t src_width, src_height;   /* the resident Split frame (no partition; layout as AIC_FRAME_OUT_SPLIT) */
    uint32_t out_width, out_height;   /* the logged size; may equal, exceed or fall below the source in either axis */
    float inverse_projection_zw[4];   /* {ipz.z, ipw.z, ipz.w, ipw.w}, as aic_reproject_desc's */
    uint32_t flags;                   /* none defined: must be 0 */
    uint32_t reserved[3];
} aic_export_desc;
typedef struct aic_export_info {
    float kernel_ms;                  /* HIP events around the launch */
    uint32_t n_surface;               /* output pixels whose exported depth is finite and > 0 */
    float depth_min, depth_max;       /* over those pixels; 0, 0 when there are none */
    uint32_t reserved[4];
} aic_export_info;
int aic_export_split(aic_ctx *ctx, const aic_export_desc *desc, const void *src_device, void *color_out /* [h][w] RGBA8, may be NULL */,
                     float *depth_out /* [h][w] f32, may be NULL */, int out_is_device, aic_export_info *info /* may be NULL */);
/* replaces: logged_image_size_policy (all-is-cubes-gpu/src/rerun_image.rs:302-311) with the area cap as a parameter, host-only, in f64: area = w * h; if
 * area <= max_area the size is returned as it is, else r = sqrt(max_area / area) and out = ceil(size * r) per axis. The reference's cap is 640 * 480:
 * (640, 480) -> (640, 480), (1920, 1080) -> (740, 416). (0, h) and (w, 0) return themselves. AIC_ERR_INVALID: a NULL out; max_area NaN or not positive. */
int aic_export_size(uint32_t width, uint32_t height, double max_area, uint32_t out[2]);

/* --- automatic exposure ---------------------------------------------------------------------- */
/* ExposureOption::Automatic: the camera's exposure follows the luminance the character sees, measured by character::exposure::State::step
 * (all-is-cubes/src/character/exposure.rs:60-151) once per simulation step. Four entry points: three restate the state and its arithmetic on the host,
 * one samples the scene on the device, next to the light volume it reads (which, once the light updater runs on the device, is nowhere else). One step
 * of the reference with view transform `vt` and time step `dt` (nothing at all when dt == 0) is
 *     aic_exposure_rays(vt.rotation, vt.translation, (s.luminance_sample_index + 1) % 100, 10, rays);
 *     aic_sample_luminance(ctx, AIC_LAYER_WORLD, 10, rays, max_steps, 0, samples);
 *     aic_exposure_advance(&s, 10, samples, dt, &exposure);        -> Camera::set_measured_exposure(exposure)
 * DESIGN.md 4.16 has the arithmetic; tests/exposure_ref.py is that text in NumPy. An aic_multi replicates the scene on every device: a host of one
 * samples through aic_multi_context(m, 0), and there is no aic_multi_* form of these calls. */
#define AIC_EXPOSURE_SAMPLES 100 /* State::luminance_samples */
#define AIC_EXPOSURE_RAYS 10     /* rays per step */
/* replaces: character::exposure::State (exposure.rs:37-48) */
typedef struct aic_exposure_state {
    float luminance_samples[100];
    uint32_t luminance_sample_index; /* the last element written */
    float exposure_log;              /* ln of the exposure */
} aic_exposure_state;
/* replaces: impl Default for State (exposure.rs:50-58): every sample 1.0, index 0, exposure_log 0. Host-only. AIC_ERR_INVALID: NULL. */
int aic_exposure_init(aic_exposure_state *s);
/* replaces: the rays of State::step (exposure.rs:85-105), host-only and in f64 in the reference's order of operations. Ray k, k < n, belongs to
 * sample index j = (first_index + k) % 100: rays[k] = {origin xyz, direction xyz} with origin = vt.transform_point3d(0, 0, 0) and direction =
 * vt.transform_vector3d((j rem 10) / 10 * 2 - 1, (j div 10) / 10 * 2 - 1, -1) -- a fixed 90 degree field of view, directions not normalised --
 * where vt = RigidTransform3D { rotation, translation }.to_transform(). AIC_ERR_INVALID: a NULL pointer (rays may be NULL when n == 0). */
int aic_exposure_rays(const double rotation_ijkr[4], const double translation[3], uint32_t first_index, uint32_t n, double *rays /* [n][6] */);
/* replaces: the sampling loop of State::step (exposure.rs:91-128) for n rays against the layer's space as last updated. Ray i = {origin, direction},
 * taken as given and not normalised, steps through Raycaster(origin, direction).within(bounds, false).take(max_steps); at each step: the cube ahead
 * outside the bounds -> the sky; a block ahead that is visible() (EvaluatedBlock::visible: a block with a voxel that is not fully transparent or emits
 * -- a voxel block whose voxels are all invisible is NOT) and Space::get_light(cube behind) -- the layer's current light volume, BlockSky::light_outside
 * for a cube outside it -- with status Visible -> out[i] = that texel's value().luminance(); the steps exhausted or the ray ended -> the sky:
 * out[i] = sky.sample(direction).luminance() (sky.rs:32-41: the octant by >= 0.0, so -0.0 is positive and NaN negative). Rgb::luminance
 * (color.rs:288-297) is g * 0.7152f + (r * 0.2126f + b * 0.0722f) in f32. max_steps: 2 * maximum_distance of LightPhysics::Rays, 0 for
 * LightPhysics::None (every sample is then the sky). Zero, NaN and infinite components are legal and sample what the reference samples.
 * flags: AIC_RAYS_DEVICE or 0 -- as for aic_trace_rays, `rays` (at a 16-byte boundary) and `out` are device pointers, nothing is staged or read back.
 * The call returns when the samples are there. It is legal while frames are in flight on any slot and disturbs none of them (it reads what they read,
 * on a stream that is none of theirs); it finishes a pending aic_evaluate_light_submit first, like every call that needs the scene, and sees every
 * scene and light write issued before it. The first call after a change of the scene makes a bitmap of the visible blocks (a read-back of the voxel
 * and palette pools if a block has voxels). AIC_ERR_INVALID: a NULL pointer with n > 0, a layer without a space, n above 1 << 20, unknown flag bits,
 * misaligned device pointers; the context stays usable. n == 0 is AIC_OK. */
int aic_sample_luminance(aic_ctx *ctx, int layer, uint32_t n, const double *rays, uint32_t max_steps, uint32_t flags, float *out /* [n] */);
/* replaces: what State::step does with its samples (exposure.rs:67-73, 94-95, 113-135) and State::exposure (exposure.rs:63-65). Host-only. dt == 0
 * changes nothing. Otherwise sample k is stored at (luminance_sample_index + 1 + k) % 100 and the index ends on the last one written; then
 * luminance_average = (the f32 sum of the 100 samples in index order) * (1.0f / 100.0f); target = compute_target_exposure(luminance_average) =
 * clamp(0.9f / l, 0.1f, 4.f) * 0.375f + 1.f * (1.f - 0.375f) (f32::clamp: NaN stays NaN); and if target is finite,
 * exposure_log += (ln(target) - exposure_log) * (float)dt * 2.0f, in that order. *exposure (may be NULL) = exp(exposure_log). ln and exp are the f64
 * functions rounded once to f32. AIC_ERR_INVALID: a NULL state, n above 100, NULL samples with n > 0, a state whose index is not below 100. */
int aic_exposure_advance(aic_exposure_state *s, uint32_t n, const float *samples, double dt, float *exposure /* may be NULL */);
/* number of rows / first rows a partition selects (host-side helper for buffer sizing) */
uint32_t aic_partition_rows(uint32_t height, const aic_partition *partition);
/* scatter compacted strips gathered from n_parts contexts back into a full frame, on device:
 * gathered = [n_parts][max_rows_per_part][width] pixels, out = [height][width]. */
int aic_assemble_strips(aic_ctx *ctx, const void *gathered_device, void *out_device, uint32_t width, uint32_t height,
                        uint32_t strip_rows, uint32_t n_parts);
/* The same de-interleave queued on the context's stream WITHOUT waiting for it: for an exchange loop that only enqueues
 * (aic_stream_wait_frame / aic_wait_event order the device side). The image is complete once the stream is (aic_synchronize, or an
 * event of the caller's recorded behind it through aic_stream). */
int aic_assemble_strips_async(aic_ctx *ctx, const void *gathered_device, void *out_device, uint32_t width, uint32_t height,
                              uint32_t strip_rows, uint32_t n_parts);
/* ... or on a stream of the caller's on the context's device (hip_stream: a hipStream_t; NULL = the context's own): the exchange step of a pipeline that
 * keeps its copies and de-interleaves off the streams the frames are traced on (aic_multi_render_submit does). */
int aic_assemble_strips_on(aic_ctx *ctx, const void *gathered_device, void *out_device, uint32_t width, uint32_t height,
                           uint32_t strip_rows, uint32_t n_parts, void *hip_stream);
/* read back the aux records of the last aic_render issued with AIC_FRAME_AUX
 * ([rows_rendered][width]). */
int aic_read_aux(aic_ctx *ctx, aic_pixel_aux *out, uint64_t n_records);
/* blocks until all work queued on the context's stream is complete */
int aic_synchronize(aic_ctx *ctx);
/* the context's HIP stream (hipStream_t) for callers that time or order work against it */
void *aic_stream(aic_ctx *ctx);
/* Everything the context queues from now on (on any of its streams) waits for `hip_event` (a hipEvent_t recorded by
 * the caller on a stream of its own, e.g. after an RCCL gather that reads or writes buffers the next frames touch):
 * orders foreign work before the context's without blocking the host. */
int aic_wait_event(aic_ctx *ctx, void *hip_event);
/* The mirror of aic_wait_event: `hip_stream` (a hipStream_t of the caller's, e.g. the stream an RCCL gather of the frame's strips is
 * issued from) waits ON THE DEVICE for the frame submitted on `slot` -- hipStreamWaitEvent on the event aic_render_submit recorded
 * behind the slot's trace. The host does not block and the slot stays occupied (aic_render_wait still collects it, later, off
 * the exchange step's path). A slot with no frame in flight is a no-op. Together the two calls hand a frame from the trace to
 * the gather and the ring slot back to the trace without a host round trip (the reference has no counterpart: its image loop,
 * renderer.rs:516-556, returns a finished image to one caller). */
int aic_stream_wait_frame(aic_ctx *ctx, uint32_t slot, void *hip_stream);

/* --- orthographic views (icons, previews) -------------------------------------------------- */
/* replaces: raytracer::ortho::render_orthographic (all-is-cubes-render/src/raytracer/ortho.rs:30-88): five pixel-perfect
 * axis-aligned views of the layer's space (top, left, front, right, bottom: MultiOrthoCamera, ortho.rs:142-200) at
 * `resolution` pixels per cube, traced with GraphicsOptions::UNALTERED_COLORS by trace_axis_aligned_ray
 * (sr.rs:126-133) and encoded with Rgba::to_srgb8; pixels between the views are transparent. out_rgba8 =
 * [*height][*width] RGBA8 (NULL: only report the size). info->cubes_traced counts every pixel's trace; the
 * reference's per-row pixel cache (ortho.rs:103-131) skips repeated voxel columns and so reports fewer steps for
 * the same image. */
int aic_ortho_image_size(const int32_t lo[3], const int32_t size[3], int resolution, uint32_t *width, uint32_t *height);
int aic_render_orthographic(aic_ctx *ctx, int layer, int resolution, void *out_rgba8, int out_is_device, uint32_t *width,
                            uint32_t *height, aic_frame_info *info);

/* --- several devices in one process ------------------------------------------------------ */
/* No reference counterpart: the reference's renderer is one object, and so is this -- an aic_multi owns one context
 * per device (ids may repeat), replicates the scene calls on all of them, and renders a frame by dealing 8-row
 * strips round-robin to the devices (rows are independent work items in the reference: renderer.rs:537-555),
 * copying each device's compact strips to device_ids[0] over its direct xGMI link (hipMemcpyPeerAsync) and
 * de-interleaving there. The multi-PROCESS form of the same partition (one rank per GPU, RCCL gather) is what
 * bench.py drives; both produce the single-device frame byte for byte. RGBA8 output only. */
typedef struct aic_multi aic_multi;
aic_multi *aic_create_multi(int n_devices, const int *device_ids, int *status);
void aic_destroy_multi(aic_multi *m);
int aic_multi_device_count(const aic_multi *m);
aic_ctx *aic_multi_context(aic_multi *m, int i);
const char *aic_multi_last_error(const aic_multi *m);
int aic_multi_upload_space(aic_multi *m, int layer, const aic_space_desc *space);
int aic_multi_clear_space(aic_multi *m, int layer);
int aic_multi_update_cubes(aic_multi *m, int layer, uint32_t n, const int32_t *xyz, const uint16_t *block_index, const uint8_t *light);
int aic_multi_update_light_volume(aic_multi *m, int layer, const uint8_t *light);
int aic_multi_replace_blocks(aic_multi *m, int layer, uint32_t n, const uint32_t *indices, const aic_block_desc *descs,
                             const uint16_t *const *voxels, const float *const *palettes);
int aic_multi_set_options(aic_multi *m, int layer, const aic_options *options);
int aic_multi_set_depth_transform(aic_multi *m, const double zw[4]);
/* out_rgba8: [height][width] RGBA8; out_is_device != 0: a device pointer on device_ids[0] */
int aic_multi_render(aic_multi *m, const aic_frame_desc *frame, void *out_rgba8, int out_is_device, aic_frame_info *info);
/* The streaming pair of the multi-device context (ABI 3), as aic_render_submit / aic_render_wait are of one context's: submit queues the frame on
 * slot 0..AIC_MULTI_MAX_IN_FLIGHT-1 of every device and returns at once -- each device traces its strips, device 0's transfer stream waits for the
 * shares on the device, copies them over the peers' links and de-interleaves --; wait blocks until that slot's frame is in out_rgba8 (a device pointer on
 * device_ids[0], or host memory: then the read-back happens in the wait) and reports it. With two or more slots in use the next frame's traces run
 * under this frame's copies: the only way a caller that renders frame after frame (all-is-cubes-desktop/src/record.rs:97-113) keeps N devices busy.
 * Scene calls (aic_multi_upload_space ...) wait for the frames in flight as the single-context ones do. aic_multi_render is submit + wait on slot 0. */
#define AIC_MULTI_MAX_IN_FLIGHT 8u
int aic_multi_render_submit(aic_multi *m, const aic_frame_desc *frame, void *out_rgba8, int out_is_device, uint32_t slot);
int aic_multi_render_wait(aic_multi *m, uint32_t slot, aic_frame_info *info);

/* --- device-side probes used by the parity tests (not part of the render path) --------- */
/* runs Raycaster::new(origin,dir)[.within(lo,hi,include_exit)] on the device, one ray,
 * and writes up to max_steps {cube[3], face, t_distance} records (raycast.rs:239-284). */
typedef struct aic_rc_step {
    int32_t cube[3];
    int32_t face;
    double t_distance;
    double intersection_point[3];
} aic_rc_step;
int aic_probe_raycast(aic_ctx *ctx, const double origin[3], const double direction[3], int use_bounds,
                      const int32_t lo[3], const int32_t hi[3], int include_exit, uint32_t max_steps,
                      aic_rc_step *out, uint32_t *n_out, int *ended);
/* the device's f32::powf as apply_transmittance uses it (raytracer_components.rs:215-258): out[i] = x[i]^y[i] */
int aic_probe_powf(aic_ctx *ctx, const float *x, const float *y, uint32_t n, float *out);
/* the device's f32::exp as distance_fog uses it (sr.rs:745-768): out[i] = e^x[i]; AIC_ERR_INVALID unless every |x[i]| < 88 */
int aic_probe_expf(aic_ctx *ctx, const float *x, uint32_t n, float *out);
/* The bloom post-process of AIC_FRAME_BLOOM on host memory: colorbuf = [height][width][4] ColorBuf l0, l1, l2, t (what AIC_FRAME_OUT_COLORBUF
 * writes) -> out_rgba8 = [height][width][4], with options' bloom_intensity, tone_mapping and maximum_intensity and the world camera's exposure.
 * Runs the chain and the composite even at intensity 0. out_mip0 (may be NULL) = the chain's result, mip 0, as f16 bits [T0y][T0x][4];
 * mip0_size (may be NULL) = {T0x, T0y}: (ceil(width / 2), ceil(height / 2)) rounded up to a multiple of 2^levels. */
int aic_probe_bloom(aic_ctx *ctx, uint32_t width, uint32_t height, const float *colorbuf, float exposure, const aic_options *options,
                    uint8_t *out_rgba8, uint16_t *out_mip0, uint32_t mip0_size[2]);
/* the device's PackedLight decode table (light/data.rs:301-354) */
int aic_probe_light_lut(aic_ctx *ctx, float out[256]);

/* ---- light propagation on the device ----
 * The light volume that the tracer reads is produced in the reference by Space's light updater
 * (all-is-cubes/src/space/light/updater.rs). These entry points run that updater against the uploaded space: the
 * priority queue and the apply step on the host, Space::compute_light (updater.rs:368-417) for a batch of queue
 * entries at a time on the device. The light volume is updated IN PLACE on the device (no aic_update_light_volume
 * round trip); aic_read_light_volume copies it out. */
typedef struct aic_light_params {
    int32_t maximum_distance; /* LightPhysics::Rays { maximum_distance } (space.rs: u8) */
    int32_t fast;             /* nonzero: Mutation::fast_evaluate_light first (updater.rs:537-581): discards the current
                                 light and queue, estimates sky light per column, queues every cube near a surface */
    int32_t epsilon;          /* Mutation::evaluate_light(epsilon, ..) (space.rs:1496-1527): stop when the queue's highest
                                 priority is at most Priority::from_difference(epsilon) */
    int32_t batch;            /* queue entries computed against one light state before any is applied: 32 = the reference
                                 built with "auto-threads" (updater.rs:231-268), 1 = without; larger = throughput */
    int32_t queue_order;      /* order of equal-priority updates: 16 or 8 = the table order of the reference's queue
                                 (hashbrown Group::WIDTH of the build target: 16 on x86-64, 8 elsewhere); 0 = first in, first out */
    int32_t n_queue;          /* when !fast: entries to ADD to the layer's queue, inserted in order (what
                                 modified_cube_needs_update, updater.rs:135-173, enqueues after a change); < 0: every cube
                                 whose texel is Uninitialized, at Priority::UNINIT */
    int32_t lanes_per_cube;   /* how compute_light is mapped to the device: 256 (or 0 = default) / 64: a block of four waves / one
                                 wave per cube walks the ray-bundle tree level by level and the contributions are added in the
                                 reference's order; 1 = one lane per cube (the plain restatement). Same results, bit for bit */
    int32_t hooks;            /* 0 in normal use. Test / experiment hooks (ABI 3; environment variables read per call until then): bit 0 = serve a call's
                                 small batches from one session kernel fed through pinned host memory (AIC_LIGHT_HOOK_SESSION; measured neutral,
                                 profiles/r04_experiments.txt J); bits 8-23 = chunks the layer's dependency pool STARTS with (0: eight per cube),
                                 to force the grow-and-recompute path */
    const int32_t *queue_cubes;      /* [n_queue][3] */
    const int32_t *queue_priorities; /* [n_queue], 0..255 */
    uint64_t max_updates;     /* stop once this many cubes were updated (checked between batches); 0 = run until done */
} aic_light_params;
#define AIC_LIGHT_HOOK_SESSION 1
#define AIC_LIGHT_HOOK_POOL_SHIFT 8
typedef struct aic_light_info {
    uint64_t updates;     /* cubes computed and applied (LightUpdatesInfo::update_count) */
    uint64_t batches;     /* device launches */
    uint64_t cost;        /* sum of ComputedLight::cost */
    double device_ms;     /* time inside the gather kernel */
    double total_ms;      /* wall time of the call */
    uint32_t queue_left;  /* entries left in the queue (at or below epsilon, or cut off by max_updates) */
    uint32_t pad;
    uint64_t bundles_visited;  /* ray-tree bundles visited by the device walk (walk_ray_tree calls that passed the weight and
                                * distance checks, updater.rs:427-530): the unit of work of the light updater's roofline (ABI 2) */
} aic_light_info;
int aic_evaluate_light(aic_ctx *ctx, int layer, const aic_light_params *params, aic_light_info *info);
/* The same update WITHOUT blocking the caller (ABI 3): aic_evaluate_light_submit copies `params` (and its queue arrays), hands the update to a worker thread
 * the context owns and returns; the update works on a spare light volume, a copy of the current one, so every frame submitted while it runs reads the
 * light as it stood. aic_evaluate_light_wait blocks until the update is done, PUBLISHES it -- the frames submitted from then on read the updated volume --
 * and reports it. A sim + render loop (Space::step's light budget, space.rs:1496-1540, then a frame) calls submit, submits its frame, and waits at the top
 * of the next step: the update's host half (queue, apply) and its launches run beside the frame instead of in front of it. One update at a time per
 * context; every other scene or light call (aic_update_cubes, aic_light_cubes_changed, aic_read_light_volume, aic_evaluate_light ...) first finishes and
 * publishes a pending update, whose report stays available to aic_evaluate_light_wait. The volume after the wait is byte for byte what the blocking call
 * produces. Nothing submitted for `layer`: the wait returns zeros. */
int aic_evaluate_light_submit(aic_ctx *ctx, int layer, const aic_light_params *params);
int aic_evaluate_light_wait(aic_ctx *ctx, int layer, aic_light_info *info);
/* *done = 0 while a submitted update of `layer` is still running, 1 otherwise (finished and waiting to be collected, or none): a loop that must not stall
 * on the light (frames at their own pace, the light a step or two behind) asks before it waits. Publishes nothing. */
int aic_evaluate_light_poll(aic_ctx *ctx, int layer, int *done);
/* After aic_update_cubes changed the blocks of these cubes: what LightStorage::modified_cube_needs_update (updater.rs:135-173) does
 * for each -- a cube that is now opaque for light gets PackedLight::OPAQUE at once, any other is queued at Priority::NEWLY_VISIBLE,
 * and so are the neighbours that are not opaque towards it. The queue is the layer's own and lives until the next
 * aic_upload_space: a following aic_evaluate_light with fast = 0 and n_queue = 0 drains it (in several calls if max_updates is
 * set: a per-frame budget, as Space::step gives its light updater). */
int aic_light_cubes_changed(aic_ctx *ctx, int layer, uint32_t n, const int32_t *xyz, int queue_order);
/* the layer's current light volume, [n cubes][4] PackedLight texels, Z-major */
int aic_read_light_volume(aic_ctx *ctx, int layer, uint8_t *out);
/* the texels of n cubes, out[n][4] (LightStorage::get, all-is-cubes/src/space/light/data.rs, over a list): served from the
 * updater's host mirror of the volume when that is current. AIC_ERR_INVALID for a cube outside the space. */
int aic_read_light_cubes(aic_ctx *ctx, int layer, uint32_t n, const int32_t *xyz, uint8_t *out);
/* Adds what the reference does not have: which light texels the UPDATER changed, for a caller that keeps a resident frame (aic_pick_stale_cubes takes the
 * answer as its light_cubes). The answer is exact: a cube is reported iff its four texel bytes in the layer's published volume differ from the baseline;
 * a texel that moved and moved back is not reported.
 * The baseline starts as the volume of aic_upload_space and follows every texel the CALLER writes itself, which are therefore never reported:
 * aic_update_light_volume, the `light` of aic_update_cubes, aic_compact; a take sets it to the current volume. The updater's writes are the apply step of
 * aic_evaluate_light, the estimate of fast = 1 (a full relight: the diff against the whole baseline) and the OPAQUE texels aic_light_cubes_changed
 * stores. The changes of an update submitted with aic_evaluate_light_submit join when it is PUBLISHED -- at aic_evaluate_light_wait or at the call that
 * ends it --, so that frames and takes agree on the volume: until then aic_light_changed_count answers for the published volume and does not wait,
 * and aic_light_changed_take, like every call that changes light state, ends the update first (its outcome stays for aic_evaluate_light_wait).
 * aic_light_changed_count: *n = the number of reported cubes, bounds (may be NULL) = their bounding box {lo x, y, z, hi x, y, z}, upper bounds
 * exclusive, all 0 when there are none; nothing is consumed.
 * aic_light_changed_take: those cubes as xyz[n][3], ascending in the volume's cube index ((x - lo.x) * size.y + (y - lo.y)) * size.z + (z - lo.z), and
 * *n_written = n; then the baseline becomes the current volume. capacity < n: AIC_ERR_INVALID, nothing written or consumed.
 * AIC_ERR_INVALID: a NULL n or n_written, a NULL xyz with capacity > 0, no space uploaded for the layer. */
int aic_light_changed_count(aic_ctx *ctx, int layer, uint64_t *n, int32_t bounds[6]);
int aic_light_changed_take(aic_ctx *ctx, int layer, uint32_t capacity, int32_t *xyz, uint32_t *n_written);
/* The propagation chart (chart/generator.rs): returns the node count; fills weights[n][6] and children[n][6] when both
 * are non-null, and the depth of the tree. Host-only: needs no device or context. */
uint32_t aic_light_chart(float *weights, uint32_t *children, uint32_t *depth);
/* test probes: the per-block derived properties the updater reads (derived.rs:78-240): out[n_blocks][32] = colour rgba,
 * 6 face colours rgba (nx ny nz px py pz), emission rgb, visible; out_opaque[n_blocks][6]. And the device's f32::log2
 * as PackedLight::scalar_in uses it (data.rs:214-218). */
int aic_probe_derived(aic_ctx *ctx, int layer, float *out, uint8_t *out_opaque);
int aic_probe_log2f(aic_ctx *ctx, const float *x, uint32_t n, float *out);
/* test hook: the layer's cube grid as it stands on the device, after the frames in flight: out_grid[n cubes], Z-major, each entry the block
 * index with -- for a block table of at most 16384 entries -- the cube's tag in bits 14-15 (block class plus one; 0 on an open cube: an
 * invisible cube inside the outermost layer whose six face neighbours are invisible). out_cls, if not NULL: the device's class table,
 * (n_blocks + 15) / 16 words of 2 bits per block index (0 invisible single voxel, 1 visible single voxel, 2 recursive). out_tagged, if not
 * NULL: 1 if the grid carries tags, 0 if it holds plain indices. A grid of no cubes writes nothing to out_grid. */
int aic_probe_cube_grid(aic_ctx *ctx, int layer, uint16_t *out_grid, uint32_t *out_cls, uint32_t *out_tagged);
/* aic_evaluate_light on the first device; the resulting light volume is handed to the others (the updater does not shard) */
int aic_multi_evaluate_light(aic_multi *m, int layer, const aic_light_params *params, aic_light_info *info);
/* aic_light_cubes_changed on the device that runs the light updater (device 0). The texels it writes there (PackedLight::OPAQUE at
 * the cubes that are now opaque) are scattered into the other devices' volumes before it returns -- n texels, not the volume -- so
 * all devices always trace the same light volume; if that hand-over fails, the whole volume goes over at the next
 * aic_multi_evaluate_light or aic_multi_render, whichever comes first. */
int aic_multi_light_cubes_changed(aic_multi *m, int layer, uint32_t n, const int32_t *xyz, int queue_order);
/* replaces: Space::compute_light::<LightUpdateCubeInfo> (all-is-cubes/src/space/mod.rs, light/updater.rs:368-417, light/debug.rs) for n cubes against
 * the layer's published light volume -- what GraphicsOptions::debug_light_rays_at_cursor draws for cursor.preceding_cube() (all-is-cubes-gpu
 * common/debug_lines.rs:47-63) -- and impl Wireframe for LightUpdateCubeInfo as a line list; DESIGN.md 4.21, tests/light_rays_ref.py is this text in
 * Python. Nothing is written to the volume and no cube is queued: the call asks, it does not update.
 * Per cube one aic_light_cube_info: `result` and `cost` are what compute_light returns for it (the texel r, g, b, status and ComputedLight::cost),
 * n_rays the records it pushed, first_ray the records of the cubes before it in the batch. Per D::push_ray (updater.rs:844-853: the hit of an opaque
 * face that ends a ray bundle) one aic_light_ray: trigger_cube = hit.cube, value_cube = hit.adjacent(), value = the stored texel read there,
 * light_from_struck_face = emission + clamped face colour reflecting that texel's value, f32 in the reference's order. A cube's records are in the
 * order the reference pushes them: walk_ray_tree's depth-first order, children in the order nx ny nz px py pz.
 * An opaque cube walks nothing: 0 rays, result and cost as the reference's (updater.rs:385-389). A cube outside the space (a cursor's preceding_cube
 * may be one) is ours to decide: AIC_LIGHT_CUBE_OUTSIDE, 0 rays, result and cost 0.
 * capacity: the records `rays` can hold. Cube k's records are stored, at rays[first_ray], iff first_ray + n_rays <= capacity, and then its flags carry
 * AIC_LIGHT_CUBE_STORED: whole cubes only, and the stored cubes are a prefix of the batch. totals[0] = all records of the batch, stored or not,
 * totals[1] = all its lines, 12 n + 29 totals[0].
 * lines: the wireframe of every STORED cube, as wireframe_vertices(v, Rgba(0.8, 0.8, 1.0, 1.0), &info) makes it: cube k's 12 + 29 n_rays lines start at
 * line 12 k + 29 first_ray (two vertices a line), so `lines` holds 2 * (12 n + 29 min(capacity, totals[0])) vertices at most. The 12 edges of
 * cube.aab().expand(0.1) in Aab::wireframe_points' order; then per record the 12 edges of value_cube.aab().expand(0.01) in that colour and the 17 lines
 * of Ray::wireframe_points (all-is-cubes-base raycast/ray.rs:115-158) for Ray::new(cube.center(), hit_point - cube.center()), hit_point the midpoint of
 * the trigger and value cubes' centres, coloured light_from_struck_face with alpha 1. All of it f64 with one rounding per operation (length =
 * sqrt(x*x + y*y + z*z) summed left to right, cross = (y*o.z - z*o.y, z*o.x - x*o.z, x*o.y - y*o.x)), the sines and cosines of k * TAU / 8 from the host's C
 * library, positions cast to f32 last. aic_light_rays_wireframe is the same text on the host for one cube: the device's lines equal it byte for byte.
 * flags: AIC_LIGHT_RAYS_DEVICE or 0 -- `rays` and `lines` are device pointers on the context's device (4-byte aligned), nothing of them is staged or
 * read back: aic_present_split_lines takes such `lines` with AIC_LINES_DEVICE. cubes, infos and totals are host memory always; each of infos, rays,
 * lines and totals may be NULL. The call returns when everything is there. Like aic_cursor_raycast it runs beside frames in flight and disturbs none of
 * them, finishes a pending aic_evaluate_light_submit first and sees every scene and light write issued before it.
 * AIC_ERR_INVALID, before anything is queued, the context still usable: NULL cubes with n > 0, unknown flag bits, a layer without a space,
 * maximum_distance outside 0..255, n above 1 << 16, misaligned device pointers. n == 0 is AIC_OK and does nothing (totals, if given, are zeroed).
 * An aic_multi replicates the scene and the light: a host of one asks through the context of its first device. */
typedef struct aic_light_cube_info {
    int32_t cube[3];
    uint8_t result[4];   /* PackedLight r, g, b, status */
    uint32_t cost;
    uint32_t n_rays;
    uint32_t first_ray;  /* exclusive prefix sum of n_rays over the batch */
    uint32_t flags;      /* AIC_LIGHT_CUBE_* */
} aic_light_cube_info;
typedef struct aic_light_ray {
    int32_t trigger_cube[3];
    int32_t value_cube[3];
    uint8_t value[4];
    float light_from_struck_face[3];
} aic_light_ray;
#define AIC_LIGHT_RAYS_DEVICE 1u  /* `rays` and `lines` are device pointers */
#define AIC_LIGHT_CUBE_STORED 1u  /* the cube's records are in `rays` (and its lines in `lines`) */
#define AIC_LIGHT_CUBE_OUTSIDE 2u /* the cube lies outside the space */
#define AIC_LIGHT_RAYS_MAX_CUBES 65536u
int aic_light_rays(aic_ctx *ctx, int layer, uint32_t n, const int32_t *cubes /* [n][3] */, int32_t maximum_distance, uint32_t flags, uint32_t capacity,
                   aic_light_cube_info *infos /* [n] */, aic_light_ray *rays /* [capacity] */, aic_line_vertex *lines, uint64_t totals[2]);
/* host-only: the most records one cube can produce with this maximum_distance, whatever the space holds. A record ends its ray bundle, so no two
 * records of a cube lie on one path from the chart's root: the bound is the number of bundles within the distance, the root apart, that have no child
 * within the distance -- counted in the chart, 602 (its rays) once the distance reaches the chart's. 0 for a maximum_distance outside 0..255. */
uint32_t aic_light_rays_bound(int32_t maximum_distance);
/* host-only: the lines of one cube from its info and its n_rays records, out[2 * (12 + 29 * n_rays)]; *n_lines = 12 + 29 * n_rays. A NULL pointer
 * (rays may be NULL when n_rays is 0): AIC_ERR_INVALID. */
int aic_light_rays_wireframe(const aic_light_cube_info *info, const aic_light_ray *rays, aic_line_vertex *out, uint32_t *n_lines);
/* What gather_debug_lines hands the lines pass when debug_light_rays_at_cursor is on (all-is-cubes-gpu common/debug_lines.rs:47-63, everything.rs:446-476):
 * the caller's n_first lines (host memory: the cursor's own wireframe, drawn first) and behind them the lines of `cube` -- cursor.preceding_cube() --
 * as aic_light_rays makes them, in ONE list in device memory the context owns. *device_lines and *n_lines are what aic_present_split_lines takes with
 * AIC_LINES_DEVICE; the list stays valid until the next call of this function or aic_destroy. The records and their lines never visit the host; info,
 * if not NULL, is the cube's. Everything aic_light_rays says of streams, pending light updates and rejections holds; also AIC_ERR_INVALID: a NULL cube,
 * device_lines or n_lines, NULL first with n_first > 0, more than AIC_LINES_MAX lines in all. */
int aic_light_rays_cursor_lines(aic_ctx *ctx, int layer, const int32_t *cube /* [3] */, int32_t maximum_distance, const aic_line_vertex *first, uint32_t n_first,
                                aic_light_cube_info *info, const aic_line_vertex **device_lines, uint32_t *n_lines);
/* Terminal frames -- replaces: the `terminal` graphics mode of the desktop program (all-is-cubes-desktop/src/terminal.rs:101-140): the raytracer with the
 * ColorCharacterBuf accumulator -- per pixel the first hit block's text and camera.post_process_color of Rgba::from of the ColorBuf (terminal.rs:341-366) --,
 * then image_patch_to_character (terminal/chars.rs:18-173), which turns each patch of 1x1, 1x2 or 2x4 pixels into one character and a colour pair under
 * TerminalOptions { colors, characters } (terminal/options.rs:15-185), and write_frame (terminal/ui.rs:300-360), which writes them as text and colour
 * escapes. Here the patch rule runs on the device, one lane per character cell, behind the trace: a frame leaves the device as 12 bytes per cell.
 * DESIGN.md 4.22 restates every operation; tests/cells_ref.py is that text in NumPy and the device equals it cell for cell, all three words.
 *
 * A cell: glyph is a Unicode scalar value (' ', '.', 'X', U+2580..U+259B, U+2800 + the Braille index) or AIC_CELL_GLYPH_BLOCK | layer << 16 | block_index,
 * "the text of that block of that layer" (the library knows no names, as it knows no font). fg and bg are kind << 24 | payload:
 *   kind 0  no colour: the Colors field is None, nothing is emitted     kind 1  Color::Reset     kind 2  Color::Black
 *   kind 3  Color::AnsiValue(n), payload n                               kind 4  Color::Rgb, payload r << 16 | g << 8 | b
 * A pixel's text follows its aic_pixel_aux record as the text renderer reads it: hit == 1 gives the block reference; else cubes_traced > 1000 'X' (an
 * approximation of Exception::Incomplete), cubes_traced > 0 ' ', else '.'. Under antialiasing the record is the first sample's, where CharacterBuf::mean
 * takes the first sample that has a hit: colours are exact under antialiasing, text at AntialiasingOption::None, the reference's default. */
#define AIC_CELLS_NAMES 0    /* CharacterMode::Names: the block's text, 1 x 1 rays per character */
#define AIC_CELLS_SHADES 1   /* CharacterMode::Shades: " ░▒▓█" by luminance, 1 x 1 */
#define AIC_CELLS_SPLIT 2    /* CharacterMode::Split: half blocks, 1 x 2 */
#define AIC_CELLS_SHAPES 3   /* CharacterMode::Shapes: eighth blocks without colour, Split's rule with, 1 x 2 */
#define AIC_CELLS_BRAILLE 4  /* CharacterMode::Braille: dot patterns, 2 x 4 */
#define AIC_CELLS_COLOR_NONE 0  /* ColorMode::None */
#define AIC_CELLS_COLOR_256 1   /* ColorMode::TwoFiftySix */
#define AIC_CELLS_COLOR_RGB 2   /* ColorMode::Rgb */
#define AIC_CELL_GLYPH_BLOCK 0x80000000u
#define AIC_CELL_COLOR_NONE 0u
#define AIC_CELL_COLOR_RESET 1u
#define AIC_CELL_COLOR_BLACK 2u
#define AIC_CELL_COLOR_ANSI 3u
#define AIC_CELL_COLOR_RGB 4u
typedef struct aic_cell {
    uint32_t glyph, fg, bg;
} aic_cell;
/* replaces: TerminalOptions::viewport_from_terminal_size (terminal/options.rs:25-38), host-only: cols and rows are raised to 1 (`size.max(size2(1, 1))`),
 * the framebuffer is cells x rays per character, the nominal size (cols * 0.5, rows * 1.0). Any output may be NULL. AIC_ERR_INVALID: cols or rows above
 * 65535 (the reference's u16), characters outside 0..4. */
int aic_cells_geometry(uint32_t cols, uint32_t rows, int32_t characters, uint32_t *width, uint32_t *height, double nominal[2]);
#define AIC_CELLS_IMAGE_DEVICE 1u    /* `image` and `aux` are device pointers on the context's device (16-byte / 8-byte aligned; f16 image 8-byte) */
#define AIC_CELLS_OUT_DEVICE 2u      /* `out` is a device pointer on the context's device (4-byte aligned) */
#define AIC_CELLS_IMAGE_F16 4u       /* the image holds four f16 per pixel (what aic_present_split writes with AIC_PRESENT_OUT_F16) instead of four f32 */
#define AIC_CELLS_POSTPROCESSED 8u   /* the image is already exposed and tone-mapped: post_process_color is skipped */
typedef struct aic_cells_desc {
    uint32_t cols, rows;        /* the grid; the image is aic_cells_geometry's framebuffer of max(cols, 1) x max(rows, 1) cells */
    int32_t characters, colors; /* AIC_CELLS_* / AIC_CELLS_COLOR_* */
    float exposure;             /* Camera::exposure() of post_process_color (camera_struct.rs:376-382); not NaN, not negative */
    int32_t tone_mapping;       /* 0 Clamp, 1 Reinhard */
    float maximum_intensity;    /* may be +inf: no tone mapping */
    uint32_t flags;             /* AIC_CELLS_* flags */
} aic_cells_desc;
/* cells per branch of image_patch_to_character taken, and colour conversions per branch of ColorMode::convert (up to two a cell) */
typedef struct aic_cells_info {
    uint32_t n_cells;
    uint32_t n_full, n_upper, n_lower, n_text, n_space;  /* Split without colour: the five arms (n_text: the `lum2 > 0.2` arm, with or without aux) */
    uint32_t n_shade;                                    /* Shades; Shapes without colour when |lum1 - lum2| < 0.05 */
    uint32_t n_rising, n_falling;                        /* Shapes without colour: lum1 < lum2, and the rest */
    uint32_t n_equal, n_unequal;                         /* Split and Shapes with colour: the two converted colours equal or not */
    uint32_t n_names, n_braille;
    uint32_t n_gray, n_cube, n_rgb;                      /* conversions: TwoFiftySix grey ramp, TwoFiftySix colour cube, Rgb */
    float kernel_ms;                                     /* HIP events around the cells kernel */
    uint32_t reserved;
} aic_cells_info;
/* replaces: image_patch_to_character for every cell of an image the caller has. image = [height][width] of four f32 (linear r, g, b, a: what
 * AIC_FRAME_OUT_LINEAR writes) or with AIC_CELLS_IMAGE_F16 four f16; alpha is never read (every pixel is Some(colour); Rgba::luminance and to_srgb8's colour
 * channels ignore it). aux = [height][width] first-hit records where the image lives, or NULL: Names is then AIC_ERR_INVALID and Split without colours
 * writes ' ' where it would have written the text. out = [rows][cols] cells (of the raised grid). The call blocks and runs on slot 0's stream.
 * AIC_ERR_INVALID, before anything is queued and with the context still usable: a NULL desc, image or out; characters or colors out of range; cols or rows
 * above 65535; unknown flag bits; tone_mapping other than 0 or 1; exposure NaN or negative; maximum_intensity NaN or negative; a misaligned device pointer;
 * a frame still occupying slot 0. */
int aic_image_cells(aic_ctx *ctx, const aic_cells_desc *desc, const void *image, const aic_pixel_aux *aux, aic_cell *out, aic_cells_info *info);
/* replaces: one frame of the terminal renderer (terminal.rs:119-137): traces `frame` as aic_render does with AIC_FRAME_OUT_LINEAR | AIC_FRAME_AUX into
 * scratch the context owns (16 + 56 bytes a pixel, kept until aic_destroy), then runs the cells kernel behind it on the context's stream. frame->width and
 * height must be aic_cells_geometry's of desc. desc->exposure, tone_mapping and maximum_intensity are NOT used: every pixel, UI pixels included, is
 * post-processed with frame->world.exposure and the world layer's options, as the reference does (terminal.rs:120-123). desc->flags must be 0;
 * out_is_device as in aic_render. The library sets no AIC_FRAME_PIXEL_CENTERS: the terminal draws through the image path. It accepts and refuses what
 * aic_render accepts and refuses, and refuses also AIC_FRAME_AUX, AIC_FRAME_OUT_LINEAR, AIC_FRAME_OUT_COLORBUF and AIC_FRAME_OUT_SPLIT set by the caller
 * and a frame size that is not the geometry's (AIC_ERR_INVALID), a partition with n_parts > 1 and AIC_FRAME_BLOOM (AIC_ERR_UNSUPPORTED). Either info may be
 * NULL. */
int aic_render_cells(aic_ctx *ctx, const aic_frame_desc *frame, const aic_cells_desc *desc, aic_cell *out, int out_is_device, aic_frame_info *frame_info,
                     aic_cells_info *cells_info);
/* replaces: TerminalWindow::write_frame with write_colored_and_measure (terminal/ui.rs:300-360, terminal/chars.rs:205-296) as a byte stream, host-only.
 * The escape text is this project's own statement (DESIGN.md 4.22 writes the format out), not a copy of what the reference's terminal library emits.
 * text (may be NULL): per layer a table of NUL-terminated UTF-8 strings and their column widths for block glyphs; a NULL table, an index beyond it or a
 * NULL string gives "#" of width 1; NULL widths mean 1 each. Every other glyph has width 1. A glyph of width w advances max(w, 1) cells and is written
 * only if w fits what is left of the row; its colour escape is written first either way, and only when the pair differs from the last one written.
 * Without AIC_CELLS_ANSI_IN_RECT a row ends with the attribute reset and "\r\n" and the colour memory is cleared; with it a row starts with a cursor
 * move to (origin[0], origin[1] + row), zero-based. The stream starts with cursor-hide and the attribute reset and ends with the reset.
 * *length is always the length needed; nothing is written past capacity; when capacity is too small the call returns AIC_ERR_INVALID and writes nothing.
 * AIC_ERR_INVALID also: NULL cells with cols * rows > 0, a NULL length, NULL out with capacity > 0, unknown flag bits. */
#define AIC_CELLS_ANSI_IN_RECT 1u
typedef struct aic_cells_text {
    const char *const *names[2];  /* per layer (AIC_LAYER_WORLD, AIC_LAYER_UI): [n_names] strings */
    const uint8_t *widths[2];     /* per layer: [n_names] column widths */
    uint32_t n_names[2];
    uint16_t origin[2];           /* AIC_CELLS_ANSI_IN_RECT: the rectangle's corner, column and row */
    uint32_t reserved;
} aic_cells_text;
int aic_cells_ansi(const aic_cell *cells, uint32_t cols, uint32_t rows, const aic_cells_text *text, uint32_t flags, char *out, uint64_t capacity,
                   uint64_t *length);

#ifdef __cplusplus
}
#endif
#endif /* AIC_HIP_H */
