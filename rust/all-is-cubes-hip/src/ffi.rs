//! Raw bindings to libaic_hip.so: one item per declaration of `include/aic_hip.h` (AIC_ABI_VERSION 3), same
//! names, same field order. Kept in step with the header by `tests/test_rust_shim.py` of the MI355X repository.
#![allow(non_camel_case_types, missing_docs, clippy::missing_safety_doc)]

use core::ffi::{c_char, c_int, c_void};

pub const AIC_ABI_VERSION: c_int = 3;
pub const AIC_OK: c_int = 0;
pub const AIC_ERR_INVALID: c_int = 1;
pub const AIC_ERR_NO_DEVICE: c_int = 2;
pub const AIC_ERR_OOM: c_int = 3;
pub const AIC_ERR_DEVICE: c_int = 4;
pub const AIC_ERR_UNSUPPORTED: c_int = 5;
pub const AIC_LAYER_WORLD: c_int = 0;
pub const AIC_LAYER_UI: c_int = 1;
pub const AIC_BLOCK_ONE: u32 = 1;
pub const AIC_BLOCK_AIR: u32 = 2;
pub const AIC_BLOCK_UNSELECTABLE: u32 = 4;
pub const AIC_BLOCK_VOXEL_SELECTABLE: u32 = 8;
pub const AIC_FLAW_UNSUPPORTED: u32 = 1;
pub const AIC_FLAW_NO_BLOOM: u32 = 2;
pub const AIC_FRAME_COUNTERS: u32 = 1;
pub const AIC_FRAME_AUX: u32 = 2;
pub const AIC_FRAME_PIXEL_CENTERS: u32 = 4;
pub const AIC_FRAME_OUT_LINEAR: u32 = 8;
pub const AIC_FRAME_OUT_COLORBUF: u32 = 16;
pub const AIC_FRAME_NO_FEEDBACK: u32 = 32;
pub const AIC_FRAME_BLOOM: u32 = 64;
pub const AIC_FRAME_OUT_SPLIT: u32 = 512;
pub const AIC_RAYS_NO_SKY: u32 = 128;
pub const AIC_RAYS_DEVICE: u32 = 256;
pub const AIC_PIXELS_DEVICE: u32 = 1;
pub const AIC_PIXELS_IN_PLACE: u32 = 2;
pub const AIC_REPROJECT_KEEP_SPLATS: u32 = 1;
pub const AIC_REPROJECT_MAX_LEVELS: u32 = 12;
pub const AIC_PRESENT_OUT_F16: u32 = 1;
pub const AIC_PRESENT_MAX_PIXELS: u64 = 2147483648;
pub const AIC_LINES_DEVICE: u32 = 1;
pub const AIC_TEXT_DEVICE: u32 = 1;
pub const AIC_LINES_MAX: u32 = 1048576;
pub const AIC_STALE_DEPTH_TEST: u32 = 1;
pub const AIC_STALE_MAX_RECTS: u32 = 4096;
pub const AIC_STALE_DEPTH_BEHIND: u32 = 2;
pub const AIC_CURSOR_MAX_LINES: u32 = 28;
pub const AIC_CURSOR_NO_BLOCK: u32 = 0xFFFF_FFFF;
pub const AIC_LIGHT_RAYS_DEVICE: u32 = 1;
pub const AIC_LIGHT_CUBE_STORED: u32 = 1;
pub const AIC_LIGHT_CUBE_OUTSIDE: u32 = 2;
pub const AIC_LIGHT_RAYS_MAX_CUBES: u32 = 65536;
pub const AIC_CELLS_NAMES: i32 = 0;
pub const AIC_CELLS_SHADES: i32 = 1;
pub const AIC_CELLS_SPLIT: i32 = 2;
pub const AIC_CELLS_SHAPES: i32 = 3;
pub const AIC_CELLS_BRAILLE: i32 = 4;
pub const AIC_CELLS_COLOR_NONE: i32 = 0;
pub const AIC_CELLS_COLOR_256: i32 = 1;
pub const AIC_CELLS_COLOR_RGB: i32 = 2;
pub const AIC_CELL_GLYPH_BLOCK: u32 = 0x8000_0000;
pub const AIC_CELL_COLOR_NONE: u32 = 0;
pub const AIC_CELL_COLOR_RESET: u32 = 1;
pub const AIC_CELL_COLOR_BLACK: u32 = 2;
pub const AIC_CELL_COLOR_ANSI: u32 = 3;
pub const AIC_CELL_COLOR_RGB: u32 = 4;
pub const AIC_CELLS_IMAGE_DEVICE: u32 = 1;
pub const AIC_CELLS_OUT_DEVICE: u32 = 2;
pub const AIC_CELLS_IMAGE_F16: u32 = 4;
pub const AIC_CELLS_POSTPROCESSED: u32 = 8;
pub const AIC_CELLS_ANSI_IN_RECT: u32 = 1;
pub const AIC_EXPOSURE_SAMPLES: u32 = 100;
pub const AIC_EXPOSURE_RAYS: u32 = 10;
pub const AIC_MAX_IN_FLIGHT: u32 = 32;
pub const AIC_MULTI_MAX_IN_FLIGHT: u32 = 8;
pub const AIC_TUNE_QUEUES_SHIFT: u32 = 0;
pub const AIC_TUNE_SUPER_SHIFT: u32 = 4;
pub const AIC_TUNE_VARIANT_SHIFT: u32 = 9;
pub const AIC_VARIANT_AUTO: u32 = 0;
pub const AIC_VARIANT_PLAIN: u32 = 1;
pub const AIC_VARIANT_EXCHANGING: u32 = 2;
pub const AIC_VARIANT_RECORDING: u32 = 3;
pub const AIC_LIGHT_HOOK_SESSION: i32 = 1;
pub const AIC_LIGHT_HOOK_POOL_SHIFT: i32 = 8;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_block_desc {
    pub resolution: i32,
    pub vlo: [i32; 3],
    pub vsize: [i32; 3],
    pub vox_off: u32,
    pub pal_off: u32,
    pub pal_len: u32,
    pub flags: u32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_space_desc {
    pub lo: [i32; 3],
    pub size: [i32; 3],
    pub block_index: *const u16,
    pub light: *const u8,
    pub n_blocks: u32,
    pub blocks: *const aic_block_desc,
    pub voxels: *const u16,
    pub n_voxels: u64,
    pub palette: *const f32,
    pub n_palette: u64,
    pub sky_kind: i32,
    pub sky: [[f32; 3]; 8],
    pub block_sky: [[u8; 4]; 7],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_options {
    pub fog: i32,
    pub transparency: i32,
    pub threshold: f32,
    pub lighting: i32,
    pub bounce_samples: i32,
    pub antialiasing: i32,
    pub debug_pixel_cost: i32,
    pub tone_mapping: i32,
    pub maximum_intensity: f32,
    pub bloom_intensity: f32,
    pub view_distance: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_camera {
    pub inverse_projection_view: [f64; 16],
    pub exposure: f32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_partition {
    pub strip_rows: u32,
    pub n_parts: u32,
    pub part: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_frame_desc {
    pub width: u32,
    pub height: u32,
    pub world: aic_camera,
    pub ui: aic_camera,
    pub backdrop: [f32; 4],
    pub partition: aic_partition,
    pub flags: u32,
    pub tuning: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_frame_info {
    pub cubes_traced: u64,
    pub n_outer: u64,
    pub n_inner: u64,
    pub n_hits: u64,
    pub n_light: u64,
    pub kernel_ms: f32,
    pub total_ms: f32,
    pub rows_rendered: u32,
    pub flaws: u32,
    pub variant: u32,
    pub tile_queues: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_reproject_desc {
    pub width: u32,
    pub height: u32,
    pub reprojection: [f32; 16],
    pub inverse_projection_zw: [f32; 4],
    pub flags: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_reproject_info {
    pub n_splats: u64,
    pub n_dropped: u64,
    pub n_gaps: u64,
    pub n_unfilled: u64,
    pub kernel_ms: f32,
    pub levels: u32,
    pub t0: [u32; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_pick_desc {
    pub width: u32,
    pub height: u32,
    pub n: u32,
    pub max_unknown: u32,
    pub skip_unknown: u64,
    pub cursor: u64,
    pub flags: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_pick_info {
    pub n_unknown: u64,
    pub next_cursor: u64,
    pub n_from_unknown: u32,
    pub n_from_order: u32,
    pub kernel_ms: f32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct aic_stale_rect {
    pub x0: u16,
    pub y0: u16,
    pub x1: u16,
    pub y1: u16,
    pub dmin: f32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_stale_desc {
    pub width: u32,
    pub height: u32,
    pub n: u32,
    pub max_stale: u32,
    pub skip_stale: u64,
    pub cursor: u64,
    pub n_rects: u32,
    pub flags: u32,
    pub rects: *const aic_stale_rect,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_stale_info {
    pub n_stale: u64,
    pub next_cursor: u64,
    pub n_from_stale: u32,
    pub n_from_order: u32,
    pub kernel_ms: f32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_stale_cubes_desc {
    pub width: u32,
    pub height: u32,
    pub n: u32,
    pub max_stale: u32,
    pub skip_stale: u64,
    pub cursor: u64,
    pub view_projection: [f64; 16],
    pub n_boxes: u32,
    pub expand: i32,
    pub n_light_cubes: u32,
    pub flags: u32,
    pub boxes: *const i32,
    pub light_cubes: *const i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_stale_cubes_info {
    pub n_stale: u64,
    pub next_cursor: u64,
    pub n_from_stale: u32,
    pub n_from_order: u32,
    pub kernel_ms: f32,
    pub reserved: u32,
    pub n_rects: u32,
    pub whole_frame: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_block_cubes_info {
    pub n_cubes: u64,
    pub n_runs: u64,
    pub bounds: [i32; 6],
    pub n_written: u32,
    pub merged: u32,
    pub kernel_ms: f32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_stale_blocks_desc {
    pub cubes: aic_stale_cubes_desc,
    pub layer: i32,
    pub n_blocks: u32,
    pub block_indices: *const u32,
    pub max_runs: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_stale_blocks_info {
    pub pick: aic_stale_cubes_info,
    pub found: aic_block_cubes_info,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct aic_stale_cube_rect {
    pub x0: u32,
    pub y0: u32,
    pub x1: u32,
    pub y1: u32,
    pub dmin: f32,
    pub dmax: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_present_desc {
    pub src_width: u32,
    pub src_height: u32,
    pub out_width: u32,
    pub out_height: u32,
    pub bloom_intensity: f32,
    pub tone_mapping: i32,
    pub maximum_intensity: f32,
    pub flags: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_present_info {
    pub kernel_ms: f32,
    pub levels: u32,
    pub t0: [u32; 2],
    pub bloomed: u32,
    pub reserved: [u32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_export_desc {
    pub src_width: u32,
    pub src_height: u32,
    pub out_width: u32,
    pub out_height: u32,
    pub inverse_projection_zw: [f32; 4],
    pub flags: u32,
    pub reserved: [u32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_export_info {
    pub kernel_ms: f32,
    pub n_surface: u32,
    pub depth_min: f32,
    pub depth_max: f32,
    pub reserved: [u32; 4],
}

/// `character::exposure::State` (exposure.rs:37-48)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_exposure_state {
    pub luminance_samples: [f32; 100],
    pub luminance_sample_index: u32,
    pub exposure_log: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct aic_line_vertex {
    pub position: [f32; 3],
    pub color: [f32; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_lines_desc {
    pub view_projection: [f32; 16],
    pub n_lines: u32,
    pub flags: u32,
    pub vertices: *const aic_line_vertex,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct aic_lines_info {
    pub n_clipped_away: u64,
    pub n_fragments: u64,
    pub n_passed: u64,
    pub n_pixels: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_text_desc {
    pub scale: [f32; 2],
    pub origin: [f32; 2],
    pub cols: u32,
    pub rows: u32,
    pub flags: u32,
    pub codes: *const u8,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_cursor_desc {
    pub cube: [i32; 3],
    pub face_entered: i32,
    pub face_selected: i32,
    pub point_entered: [f64; 3],
    pub distance_to_point: f64,
    pub voxel_lo: [i32; 3],
    pub voxel_size: [i32; 3],
    pub resolution: i32,
    pub reserved: i32,
}

/// One record of `aic_cursor_raycast`: 144 bytes, all zero for the reference's `None`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_cursor_hit {
    pub cursor: aic_cursor_desc,
    pub hit: i32,
    pub block_index: u32,
    pub voxel: [i32; 3],
    pub has_preceding: i32,
    pub preceding_cube: [i32; 3],
    pub preceding_block_index: u32,
    pub light_hit: [u8; 4],
    pub light_preceding: [u8; 4],
    pub steps: u32,
    pub reserved_hit: u32,
}

/// What `aic_light_rays` answers per cube: 32 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct aic_light_cube_info {
    pub cube: [i32; 3],
    pub result: [u8; 4],
    pub cost: u32,
    pub n_rays: u32,
    pub first_ray: u32,
    pub flags: u32,
}

/// One `LightUpdateRayInfo` of `aic_light_rays`: 40 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct aic_light_ray {
    pub trigger_cube: [i32; 3],
    pub value_cube: [i32; 3],
    pub value: [u8; 4],
    pub light_from_struck_face: [f32; 3],
}

/// One character cell of a terminal frame (`aic_image_cells`, `aic_render_cells`): 12 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct aic_cell {
    pub glyph: u32,
    pub fg: u32,
    pub bg: u32,
}

/// `TerminalOptions` and the grid, with the post-processing `aic_image_cells` applies.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_cells_desc {
    pub cols: u32,
    pub rows: u32,
    pub characters: i32,
    pub colors: i32,
    pub exposure: f32,
    pub tone_mapping: i32,
    pub maximum_intensity: f32,
    pub flags: u32,
}

/// Cells per branch of `image_patch_to_character`, colour conversions per branch of `ColorMode::convert`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_cells_info {
    pub n_cells: u32,
    pub n_full: u32,
    pub n_upper: u32,
    pub n_lower: u32,
    pub n_text: u32,
    pub n_space: u32,
    pub n_shade: u32,
    pub n_rising: u32,
    pub n_falling: u32,
    pub n_equal: u32,
    pub n_unequal: u32,
    pub n_names: u32,
    pub n_braille: u32,
    pub n_gray: u32,
    pub n_cube: u32,
    pub n_rgb: u32,
    pub kernel_ms: f32,
    pub reserved: u32,
}

/// The names tables and the rectangle's corner `aic_cells_ansi` takes.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_cells_text {
    pub names: [*const *const c_char; 2],
    pub widths: [*const u8; 2],
    pub n_names: [u32; 2],
    pub origin: [u16; 2],
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_pixel_aux {
    pub hit: i32,
    pub cube: [i32; 3],
    pub voxel: [i32; 3],
    pub resolution: i32,
    pub face: i32,
    pub block_index: i32,
    pub cubes_traced: u32,
    pub layer: u32,
    pub t_distance: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_rc_step {
    pub cube: [i32; 3],
    pub face: i32,
    pub t_distance: f64,
    pub intersection_point: [f64; 3],
}

#[repr(C)]
pub struct aic_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct aic_multi {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct aic_light_params {
    pub maximum_distance: i32,
    pub fast: i32,
    pub epsilon: i32,
    pub batch: i32,
    pub queue_order: i32,
    pub n_queue: i32,
    pub lanes_per_cube: i32,
    pub hooks: i32,
    pub queue_cubes: *const i32,
    pub queue_priorities: *const i32,
    pub max_updates: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aic_light_info {
    pub updates: u64,
    pub batches: u64,
    pub cost: u64,
    pub device_ms: f64,
    pub total_ms: f64,
    pub queue_left: u32,
    pub pad: u32,
    pub bundles_visited: u64,
}

unsafe extern "C" {
    pub fn aic_create(device_id: c_int, status: *mut c_int) -> *mut aic_ctx;
    pub fn aic_destroy(ctx: *mut aic_ctx);
    pub fn aic_last_error(ctx: *const aic_ctx) -> *const c_char;
    pub fn aic_abi_version() -> c_int;
    pub fn aic_device_name(ctx: *const aic_ctx, buf: *mut c_char, buf_len: u32) -> c_int;
    pub fn aic_upload_space(ctx: *mut aic_ctx, layer: c_int, space: *const aic_space_desc) -> c_int;
    pub fn aic_clear_space(ctx: *mut aic_ctx, layer: c_int) -> c_int;
    pub fn aic_update_cubes(ctx: *mut aic_ctx, layer: c_int, n: u32, xyz: *const i32, block_index: *const u16, light: *const u8) -> c_int;
    pub fn aic_update_light_volume(ctx: *mut aic_ctx, layer: c_int, light: *const u8) -> c_int;
    pub fn aic_replace_block(ctx: *mut aic_ctx, layer: c_int, index: u32, desc: *const aic_block_desc, voxels: *const u16, palette: *const f32) -> c_int;
    pub fn aic_replace_blocks(ctx: *mut aic_ctx, layer: c_int, n: u32, indices: *const u32, descs: *const aic_block_desc, voxels: *const *const u16, palettes: *const *const f32) -> c_int;
    pub fn aic_compact(ctx: *mut aic_ctx, layer: c_int) -> c_int;
    pub fn aic_set_options(ctx: *mut aic_ctx, layer: c_int, options: *const aic_options) -> c_int;
    pub fn aic_set_depth_transform(ctx: *mut aic_ctx, zw: *const f64) -> c_int;
    pub fn aic_render(ctx: *mut aic_ctx, frame: *const aic_frame_desc, out_rgba8: *mut c_void, out_is_device: c_int, info: *mut aic_frame_info) -> c_int;
    pub fn aic_render_submit(ctx: *mut aic_ctx, frame: *const aic_frame_desc, out_device: *mut c_void, slot: u32) -> c_int;
    pub fn aic_render_wait(ctx: *mut aic_ctx, slot: u32, info: *mut aic_frame_info) -> c_int;
    pub fn aic_render_submit_batch(ctx: *mut aic_ctx, n_frames: u32, frames: *const aic_frame_desc, out_devices: *const *mut c_void, slot: u32) -> c_int;
    pub fn aic_render_wait_batch(ctx: *mut aic_ctx, slot: u32, n_frames: u32, infos: *mut aic_frame_info) -> c_int;
    pub fn aic_trace_patches(ctx: *mut aic_ctx, frame: *const aic_frame_desc, n: u32, rects: *const f64, out_rgba8: *mut c_void, aux: *mut aic_pixel_aux, info: *mut aic_frame_info) -> c_int;
    pub fn aic_partition_rows(height: u32, partition: *const aic_partition) -> u32;
    pub fn aic_assemble_strips(ctx: *mut aic_ctx, gathered_device: *const c_void, out_device: *mut c_void, width: u32, height: u32, strip_rows: u32, n_parts: u32) -> c_int;
    pub fn aic_assemble_strips_async(ctx: *mut aic_ctx, gathered_device: *const c_void, out_device: *mut c_void, width: u32, height: u32, strip_rows: u32, n_parts: u32) -> c_int;
    pub fn aic_assemble_strips_on(ctx: *mut aic_ctx, gathered_device: *const c_void, out_device: *mut c_void, width: u32, height: u32, strip_rows: u32, n_parts: u32, hip_stream: *mut c_void) -> c_int;
    pub fn aic_trace_rays(ctx: *mut aic_ctx, layer: c_int, n: u32, rays: *const f64, flags: u32, exposure: f32, out: *mut c_void, aux: *mut aic_pixel_aux, info: *mut aic_frame_info) -> c_int;
    pub fn aic_trace_pixels(ctx: *mut aic_ctx, frame: *const aic_frame_desc, n: u32, pixels: *const u32, mode: u32, out: *mut c_void, aux: *mut aic_pixel_aux, info: *mut aic_frame_info) -> c_int;
    pub fn aic_reproject_split(ctx: *mut aic_ctx, desc: *const aic_reproject_desc, src_device: *const c_void, dst_device: *mut c_void, info: *mut aic_reproject_info) -> c_int;
    pub fn aic_reproject_geometry(width: u32, height: u32, levels: *mut u32, t0: *mut u32, scratch_bytes: *mut u64) -> c_int;
    pub fn aic_pick_pixels(ctx: *mut aic_ctx, desc: *const aic_pick_desc, order_device: *const u32, pixels_out_device: *mut u32, info: *mut aic_pick_info) -> c_int;
    pub fn aic_stale_rects(view_projection: *const f64, width: u32, height: u32, n_boxes: u32, boxes: *const i32, expand: i32, out: *mut aic_stale_rect) -> c_int;
    pub fn aic_pick_stale(
        ctx: *mut aic_ctx,
        desc: *const aic_stale_desc,
        src_device: *const c_void,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        info: *mut aic_stale_info,
    ) -> c_int;
    pub fn aic_pick_stale_cubes(
        ctx: *mut aic_ctx,
        desc: *const aic_stale_cubes_desc,
        src_device: *const c_void,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        info: *mut aic_stale_cubes_info,
    ) -> c_int;
    pub fn aic_probe_stale_cube_rects(ctx: *mut aic_ctx, desc: *const aic_stale_cubes_desc, out: *mut aic_stale_cube_rect) -> c_int;
    pub fn aic_find_block_cubes(
        ctx: *mut aic_ctx,
        layer: c_int,
        n_blocks: u32,
        block_indices: *const u32,
        capacity: u32,
        out_boxes: *mut i32,
        info: *mut aic_block_cubes_info,
    ) -> c_int;
    pub fn aic_pick_stale_blocks(
        ctx: *mut aic_ctx,
        desc: *const aic_stale_blocks_desc,
        src_device: *const c_void,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        info: *mut aic_stale_blocks_info,
    ) -> c_int;
    pub fn aic_replace_cube_grid(
        ctx: *mut aic_ctx,
        layer: c_int,
        block_index_device: *const u16,
        light_device: *const u8,
        capacity: u32,
        out_boxes: *mut i32,
        info: *mut aic_block_cubes_info,
    ) -> c_int;
    pub fn aic_copy_cube_grid(ctx: *mut aic_ctx, layer: c_int, out_device: *mut u16, light_out_device: *mut u8) -> c_int;
    pub fn aic_update_light_volume_device(ctx: *mut aic_ctx, layer: c_int, light_device: *const u8) -> c_int;
    pub fn aic_light_changed_count(ctx: *mut aic_ctx, layer: c_int, n: *mut u64, bounds: *mut i32) -> c_int;
    pub fn aic_light_changed_take(ctx: *mut aic_ctx, layer: c_int, capacity: u32, xyz: *mut i32, n_written: *mut u32) -> c_int;
    pub fn aic_present_split(ctx: *mut aic_ctx, desc: *const aic_present_desc, src_device: *const c_void, out: *mut c_void, out_is_device: c_int, info: *mut aic_present_info) -> c_int;
    pub fn aic_export_split(ctx: *mut aic_ctx, desc: *const aic_export_desc, src_device: *const c_void, color_out: *mut c_void, depth_out: *mut f32, out_is_device: c_int, info: *mut aic_export_info) -> c_int;
    pub fn aic_export_size(width: u32, height: u32, max_area: f64, out: *mut u32) -> c_int;
    pub fn aic_exposure_init(s: *mut aic_exposure_state) -> c_int;
    pub fn aic_exposure_rays(rotation_ijkr: *const f64, translation: *const f64, first_index: u32, n: u32, rays: *mut f64) -> c_int;
    pub fn aic_sample_luminance(ctx: *mut aic_ctx, layer: c_int, n: u32, rays: *const f64, max_steps: u32, flags: u32, out: *mut f32) -> c_int;
    pub fn aic_exposure_advance(s: *mut aic_exposure_state, n: u32, samples: *const f32, dt: f64, exposure: *mut f32) -> c_int;
    pub fn aic_present_geometry(src_w: u32, src_h: u32, out_w: u32, out_h: u32, levels: *mut u32, t0: *mut u32, scratch_bytes: *mut u64) -> c_int;
    pub fn aic_present_split_lines(ctx: *mut aic_ctx, desc: *const aic_present_desc, lines: *const aic_lines_desc, src_device: *const c_void, out: *mut c_void, out_is_device: c_int, info: *mut aic_present_info, lines_info: *mut aic_lines_info) -> c_int;
    pub fn aic_present_lines_scratch(src_w: u32, src_h: u32, out_w: u32, out_h: u32, n_lines: u32, bytes: *mut u64) -> c_int;
    pub fn aic_cursor_wireframe(cursor: *const aic_cursor_desc, out: *mut aic_line_vertex, n_lines: *mut u32) -> c_int;
    pub fn aic_cursor_raycast(ctx: *mut aic_ctx, layer: c_int, n: u32, rays: *const f64, maximum_distance: f64, flags: u32, out: *mut aic_cursor_hit) -> c_int;
    pub fn aic_light_rays(ctx: *mut aic_ctx, layer: c_int, n: u32, cubes: *const i32, maximum_distance: i32, flags: u32, capacity: u32, infos: *mut aic_light_cube_info, rays: *mut aic_light_ray, lines: *mut aic_line_vertex, totals: *mut u64) -> c_int;
    pub fn aic_light_rays_bound(maximum_distance: i32) -> u32;
    pub fn aic_light_rays_wireframe(info: *const aic_light_cube_info, rays: *const aic_light_ray, out: *mut aic_line_vertex, n_lines: *mut u32) -> c_int;
    pub fn aic_light_rays_cursor_lines(ctx: *mut aic_ctx, layer: c_int, cube: *const i32, maximum_distance: i32, first: *const aic_line_vertex, n_first: u32, info: *mut aic_light_cube_info, device_lines: *mut *const aic_line_vertex, n_lines: *mut u32) -> c_int;
    pub fn aic_cells_geometry(cols: u32, rows: u32, characters: i32, width: *mut u32, height: *mut u32, nominal: *mut f64) -> c_int;
    pub fn aic_image_cells(ctx: *mut aic_ctx, desc: *const aic_cells_desc, image: *const c_void, aux: *const aic_pixel_aux, out: *mut aic_cell, info: *mut aic_cells_info) -> c_int;
    pub fn aic_render_cells(ctx: *mut aic_ctx, frame: *const aic_frame_desc, desc: *const aic_cells_desc, out: *mut aic_cell, out_is_device: c_int, frame_info: *mut aic_frame_info, cells_info: *mut aic_cells_info) -> c_int;
    pub fn aic_cells_ansi(cells: *const aic_cell, cols: u32, rows: u32, text: *const aic_cells_text, flags: u32, out: *mut c_char, capacity: u64, length: *mut u64) -> c_int;
    pub fn aic_set_text_font(ctx: *mut aic_ctx, atlas_rgba8: *const u8, cell_width: u32, cell_height: u32, cell_margin: u32) -> c_int;
    pub fn aic_text_geometry(nominal_width: f64, nominal_height: f64, cell_width: u32, cell_height: u32, cell_margin: u32, origin_px: *const f64, cols: *mut u32, rows: *mut u32, scale: *mut f32, origin: *mut f32) -> c_int;
    pub fn aic_text_layout(utf8: *const c_char, len: u64, cols: u32, rows: u32, codes: *mut u8, used: *mut u32) -> c_int;
    pub fn aic_present_split_text(ctx: *mut aic_ctx, desc: *const aic_present_desc, lines: *const aic_lines_desc, text: *const aic_text_desc, src_device: *const c_void, out: *mut c_void, out_is_device: c_int, info: *mut aic_present_info, lines_info: *mut aic_lines_info) -> c_int;
    pub fn aic_pixel_order(width: u32, height: u32, order: *mut u32, central: *mut u32, cycle_length: *mut u64) -> c_int;
    pub fn aic_read_aux(ctx: *mut aic_ctx, out: *mut aic_pixel_aux, n_records: u64) -> c_int;
    pub fn aic_synchronize(ctx: *mut aic_ctx) -> c_int;
    pub fn aic_stream(ctx: *mut aic_ctx) -> *mut c_void;
    pub fn aic_wait_event(ctx: *mut aic_ctx, hip_event: *mut c_void) -> c_int;
    pub fn aic_stream_wait_frame(ctx: *mut aic_ctx, slot: u32, hip_stream: *mut c_void) -> c_int;
    pub fn aic_ortho_image_size(lo: *const i32, size: *const i32, resolution: c_int, width: *mut u32, height: *mut u32) -> c_int;
    pub fn aic_render_orthographic(ctx: *mut aic_ctx, layer: c_int, resolution: c_int, out_rgba8: *mut c_void, out_is_device: c_int, width: *mut u32, height: *mut u32, info: *mut aic_frame_info) -> c_int;
    pub fn aic_create_multi(n_devices: c_int, device_ids: *const c_int, status: *mut c_int) -> *mut aic_multi;
    pub fn aic_destroy_multi(m: *mut aic_multi);
    pub fn aic_multi_device_count(m: *const aic_multi) -> c_int;
    pub fn aic_multi_context(m: *mut aic_multi, i: c_int) -> *mut aic_ctx;
    pub fn aic_multi_last_error(m: *const aic_multi) -> *const c_char;
    pub fn aic_multi_upload_space(m: *mut aic_multi, layer: c_int, space: *const aic_space_desc) -> c_int;
    pub fn aic_multi_clear_space(m: *mut aic_multi, layer: c_int) -> c_int;
    pub fn aic_multi_update_cubes(m: *mut aic_multi, layer: c_int, n: u32, xyz: *const i32, block_index: *const u16, light: *const u8) -> c_int;
    pub fn aic_multi_update_light_volume(m: *mut aic_multi, layer: c_int, light: *const u8) -> c_int;
    pub fn aic_multi_replace_blocks(m: *mut aic_multi, layer: c_int, n: u32, indices: *const u32, descs: *const aic_block_desc, voxels: *const *const u16, palettes: *const *const f32) -> c_int;
    pub fn aic_multi_set_options(m: *mut aic_multi, layer: c_int, options: *const aic_options) -> c_int;
    pub fn aic_multi_set_depth_transform(m: *mut aic_multi, zw: *const f64) -> c_int;
    pub fn aic_multi_render(m: *mut aic_multi, frame: *const aic_frame_desc, out_rgba8: *mut c_void, out_is_device: c_int, info: *mut aic_frame_info) -> c_int;
    pub fn aic_multi_render_submit(m: *mut aic_multi, frame: *const aic_frame_desc, out_rgba8: *mut c_void, out_is_device: c_int, slot: u32) -> c_int;
    pub fn aic_multi_render_wait(m: *mut aic_multi, slot: u32, info: *mut aic_frame_info) -> c_int;
    pub fn aic_probe_raycast(ctx: *mut aic_ctx, origin: *const f64, direction: *const f64, use_bounds: c_int, lo: *const i32, hi: *const i32, include_exit: c_int, max_steps: u32, out: *mut aic_rc_step, n_out: *mut u32, ended: *mut c_int) -> c_int;
    pub fn aic_probe_powf(ctx: *mut aic_ctx, x: *const f32, y: *const f32, n: u32, out: *mut f32) -> c_int;
    pub fn aic_probe_expf(ctx: *mut aic_ctx, x: *const f32, n: u32, out: *mut f32) -> c_int;
    pub fn aic_probe_bloom(ctx: *mut aic_ctx, width: u32, height: u32, colorbuf: *const f32, exposure: f32, options: *const aic_options, out_rgba8: *mut u8, out_mip0: *mut u16, mip0_size: *mut u32) -> c_int;
    pub fn aic_probe_light_lut(ctx: *mut aic_ctx, out: *mut f32) -> c_int;
    // light propagation on the device (Space::evaluate_light / fast_evaluate_light)
    pub fn aic_evaluate_light(ctx: *mut aic_ctx, layer: c_int, params: *const aic_light_params, info: *mut aic_light_info) -> c_int;
    pub fn aic_evaluate_light_submit(ctx: *mut aic_ctx, layer: c_int, params: *const aic_light_params) -> c_int;
    pub fn aic_evaluate_light_wait(ctx: *mut aic_ctx, layer: c_int, info: *mut aic_light_info) -> c_int;
    pub fn aic_evaluate_light_poll(ctx: *mut aic_ctx, layer: c_int, done: *mut c_int) -> c_int;
    pub fn aic_light_cubes_changed(ctx: *mut aic_ctx, layer: c_int, n: u32, xyz: *const i32, queue_order: c_int) -> c_int;
    pub fn aic_read_light_volume(ctx: *mut aic_ctx, layer: c_int, out: *mut u8) -> c_int;
    pub fn aic_read_light_cubes(ctx: *mut aic_ctx, layer: c_int, n: u32, xyz: *const i32, out: *mut u8) -> c_int;
    pub fn aic_light_chart(weights: *mut f32, children: *mut u32, depth: *mut u32) -> u32;
    pub fn aic_probe_derived(ctx: *mut aic_ctx, layer: c_int, out: *mut f32, out_opaque: *mut u8) -> c_int;
    pub fn aic_probe_log2f(ctx: *mut aic_ctx, x: *const f32, n: u32, out: *mut f32) -> c_int;
    pub fn aic_probe_cube_grid(ctx: *mut aic_ctx, layer: c_int, out_grid: *mut u16, out_cls: *mut u32, out_tagged: *mut u32) -> c_int;
    pub fn aic_multi_evaluate_light(m: *mut aic_multi, layer: c_int, params: *const aic_light_params, info: *mut aic_light_info) -> c_int;
    pub fn aic_multi_light_cubes_changed(m: *mut aic_multi, layer: c_int, n: u32, xyz: *const i32, queue_order: c_int) -> c_int;
}
