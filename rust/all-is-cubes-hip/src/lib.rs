//! `HeadlessRenderer` for all-is-cubes on an AMD MI355X: the CPU raytracer of `all-is-cubes-render`
//! (`RtRenderer` / `SpaceRaytracer`) replaced by the HIP kernel behind `libaic_hip.so`.
//!
//! This crate holds on the host exactly what `RtRenderer` holds -- the `StandardCameras`, the size policy and one
//! change listener per layer (the `SpaceChange` filter of raytracer/updating.rs:200-219) -- and forwards snapshots and
//! deltas through the C ABI instead of mutating a `SpaceRaytracer`:
//!
//! | reference                                              | here                                   |
//! |--------------------------------------------------------|----------------------------------------|
//! | `RtRenderer::new` (renderer.rs:65-81)                  | `HipRtRenderer::new` -> `aic_create`   |
//! | `UpdatingSpaceRaytracer::update`, everything (121-131) | `aic_upload_space`                     |
//! | ... blocks (139-153)                                   | `aic_replace_blocks`                   |
//! | ... cubes (155-166)                                    | `aic_update_cubes`                     |
//! | `RtRenderer::draw_rgba` (renderer.rs:282-308)          | `aic_render` / `aic_multi_render`      |
//! | `draw_info_text` (renderer.rs:659-683)                 | the same few lines, on the host        |
//!
//! One renderer may span several GPUs of a node ([`HipRtRenderer::with_devices`]): the scene is replicated, every device
//! traces its interleaved 8-row strips and device 0 assembles the frame (`aic_create_multi`, csrc/aic_multi.cpp).
//! [`HipRtRenderer::set_device_light`] hands the light itself over to the device: block edits are queued there
//! (`aic_light_cubes_changed`) and [`HipRtRenderer::evaluate_light_budgeted`] advances the light between frames.
//!
//! With `AIC_DUMP=path` in the environment the library records every call it receives; the recording replays on
//! a machine without the Rust toolchain (`python -m all_is_cubes_amd.replay path` in the MI355X repository) -- that is
//! how a real Atrium / DemoCity scene reaches its benchmark and parity tests.
//!
//! NOTE: written against all-is-cubes 0.10.0. THIS CRATE HAS NEVER BEEN COMPILED: the repository that carries it has no Rust
//! toolchain (tests/test_rust_shim.py only keeps `ffi.rs` in step with include/aic_hip.h). Expect to adjust imports and
//! signatures to the workspace it is dropped into; the C++ host mirror (all_is_cubes_amd/host/) is the tested twin of this
//! file, function for function.

#![warn(missing_docs)]

use std::ffi::CStr;
use std::ptr::NonNull;
use std::sync::{Arc, Mutex};

use all_is_cubes::character::Cursor;
use all_is_cubes::listen::{self, Listen as _};
use all_is_cubes::math::{Cube, Rgba, ZeroOne};
use all_is_cubes::space::{BlockIndex, Space, SpaceChange};
use all_is_cubes::text;
use all_is_cubes::universe;
use all_is_cubes::universe::{Handle, ReadTicket};
use all_is_cubes_render::camera::{
    AntialiasingOption, Camera, FogOption, GraphicsOptions, Layers, LightingOption, StandardCameras, ToneMappingOperator,
    TransparencyOption, ViewTransform, Viewport,
};
use all_is_cubes_render::{Flaws, HeadlessRenderer, RenderError, Rendering};
use futures_core::future::BoxFuture;

pub mod ffi;
mod flatten;

use flatten::{FlatSpace, flatten_block, gather_cubes};

/// What `SrtTodo` is in the reference (updating.rs:174-219): the changes not yet forwarded to the device.
#[derive(Debug, Default)]
struct Todo {
    everything: bool,
    blocks: std::collections::HashSet<BlockIndex>,
    cubes: std::collections::HashSet<Cube>,
}

impl listen::Store<SpaceChange> for Todo {
    fn receive(&mut self, messages: &[SpaceChange]) {
        for message in messages {
            match *message {
                SpaceChange::EveryBlock => {
                    self.everything = true;
                    self.blocks.clear();
                    self.cubes.clear();
                }
                SpaceChange::CubeLight { cube, .. } | SpaceChange::CubeBlock { cube, .. } => {
                    self.cubes.insert(cube);
                }
                SpaceChange::BlockIndex(index) | SpaceChange::BlockEvaluation(index) => {
                    self.blocks.insert(index);
                }
                SpaceChange::Physics => {}
            }
        }
    }
}

struct LayerSync {
    space: Handle<Space>,
    todo: listen::StoreLock<Todo>,
    listening: bool,
    n_blocks: usize,
    /// the block indices the last `sync_layer` re-sent because their definition changed (`todo.blocks`): what `pick_stale_blocks` takes
    resent_blocks: Vec<u32>,
}

/// Renderer-specific diagnostic information: the device's `RaytraceInfo` sums and kernel time.
#[derive(Clone, Copy, Debug)]
pub struct HipInfo(pub ffi::aic_frame_info);
impl core::fmt::Display for HipInfo {
    fn fmt(&self, f: &mut core::fmt::Formatter<'_>) -> core::fmt::Result {
        write!(f, "{} cubes traced, kernel {:.3} ms", self.0.cubes_traced, self.0.kernel_ms)
    }
}

/// One context per HIP device (`aic_create`), or the single-process multi-device context (`aic_create_multi`).
#[derive(Clone, Copy)]
enum Device {
    One(NonNull<ffi::aic_ctx>),
    Many(NonNull<ffi::aic_multi>),
}

impl Device {
    fn check(self, rc: core::ffi::c_int) -> Result<(), RenderError> {
        if rc == ffi::AIC_OK {
            return Ok(());
        }
        // SAFETY: both return a NUL-terminated string owned by the context
        let message = unsafe {
            CStr::from_ptr(match self {
                Device::One(c) => ffi::aic_last_error(c.as_ptr()),
                Device::Many(m) => ffi::aic_multi_last_error(m.as_ptr()),
            })
        }
        .to_string_lossy()
        .into_owned();
        match rc {
            // the reference asserts on the same conditions (e.g. output length, renderer.rs:193-197)
            ffi::AIC_ERR_INVALID => panic!("libaic_hip rejected a call: {message}"),
            // RenderError has no device variant yet (lib.rs:46-54 "TODO: add errors for out of memory, lost GPU");
            // until it does, a lost device is reported the way an unreadable scene is. (Whether `HandleError` can be
            // built from a message outside its crate is unchecked -- this file was never compiled: a maintainer adds the
            // RenderError variant that TODO asks for.)
            _ => {
                log::error!("libaic_hip: {message}");
                Err(RenderError::Read(all_is_cubes::universe::HandleError::from_message(message)))
            }
        }
    }
    /// The context the light updater runs on (a sequential relaxation: it does not shard; csrc/aic_multi.cpp).
    #[allow(dead_code)]
    fn first_ctx(self) -> *mut ffi::aic_ctx {
        match self {
            Device::One(c) => c.as_ptr(),
            // SAFETY: a live multi context has at least one device
            Device::Many(m) => unsafe { ffi::aic_multi_context(m.as_ptr(), 0) },
        }
    }
    // SAFETY (every method below): the context is live, the borrowed arguments outlive the call, the library copies them
    fn upload_space(self, layer: core::ffi::c_int, desc: &ffi::aic_space_desc) -> Result<(), RenderError> {
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_upload_space(c.as_ptr(), layer, desc),
                Device::Many(m) => ffi::aic_multi_upload_space(m.as_ptr(), layer, desc),
            }
        })
    }
    fn clear_space(self, layer: core::ffi::c_int) -> Result<(), RenderError> {
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_clear_space(c.as_ptr(), layer),
                Device::Many(m) => ffi::aic_multi_clear_space(m.as_ptr(), layer),
            }
        })
    }
    fn replace_blocks(
        self,
        layer: core::ffi::c_int,
        indices: &[u32],
        descs: &[ffi::aic_block_desc],
        voxels: &[*const u16],
        palettes: &[*const f32],
    ) -> Result<(), RenderError> {
        let n = indices.len() as u32;
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_replace_blocks(c.as_ptr(), layer, n, indices.as_ptr(), descs.as_ptr(), voxels.as_ptr(), palettes.as_ptr()),
                Device::Many(m) => ffi::aic_multi_replace_blocks(m.as_ptr(), layer, n, indices.as_ptr(), descs.as_ptr(), voxels.as_ptr(), palettes.as_ptr()),
            }
        })
    }
    /// `light` = None: block indices only (the light of these cubes is the device's business, see `set_device_light`).
    fn update_cubes(self, layer: core::ffi::c_int, xyz: &[i32], idx: &[u16], light: Option<&[u8]>) -> Result<(), RenderError> {
        let n = idx.len() as u32;
        let light = light.map_or(core::ptr::null(), <[u8]>::as_ptr);
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_update_cubes(c.as_ptr(), layer, n, xyz.as_ptr(), idx.as_ptr(), light),
                Device::Many(m) => ffi::aic_multi_update_cubes(m.as_ptr(), layer, n, xyz.as_ptr(), idx.as_ptr(), light),
            }
        })
    }
    fn set_options(self, layer: core::ffi::c_int, options: &ffi::aic_options) -> Result<(), RenderError> {
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_set_options(c.as_ptr(), layer, options),
                Device::Many(m) => ffi::aic_multi_set_options(m.as_ptr(), layer, options),
            }
        })
    }
    fn render(self, frame: &ffi::aic_frame_desc, out: &mut [[u8; 4]], info: &mut ffi::aic_frame_info) -> Result<(), RenderError> {
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_render(c.as_ptr(), frame, out.as_mut_ptr().cast(), 0, info),
                Device::Many(m) => ffi::aic_multi_render(m.as_ptr(), frame, out.as_mut_ptr().cast(), 0, info),
            }
        })
    }
    fn evaluate_light(self, layer: core::ffi::c_int, params: &ffi::aic_light_params, info: &mut ffi::aic_light_info) -> Result<(), RenderError> {
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_evaluate_light(c.as_ptr(), layer, params, info),
                // runs on device 0 and hands the resulting volume to the others
                Device::Many(m) => ffi::aic_multi_evaluate_light(m.as_ptr(), layer, params, info),
            }
        })
    }
    /// `aic_evaluate_light_submit` / `_wait`: the update on the context's worker thread, published by the wait (single device only:
    /// the multi-device context runs the updater on device 0 and hands the volume over, which is a blocking step).
    fn evaluate_light_submit(self, layer: core::ffi::c_int, params: &ffi::aic_light_params) -> Result<bool, RenderError> {
        match self {
            // SAFETY: live handle; the library copies `params` before it returns
            Device::One(c) => self.check(unsafe { ffi::aic_evaluate_light_submit(c.as_ptr(), layer, params) }).map(|()| true),
            Device::Many(_) => Ok(false),
        }
    }
    fn evaluate_light_wait(self, layer: core::ffi::c_int, info: &mut ffi::aic_light_info) -> Result<(), RenderError> {
        match self {
            // SAFETY: live handle, `info` is a valid out-pointer
            Device::One(c) => self.check(unsafe { ffi::aic_evaluate_light_wait(c.as_ptr(), layer, info) }),
            Device::Many(_) => Ok(()),
        }
    }
    /// `aic_light_cubes_changed` for cubes whose block `update_cubes` just changed (updater.rs:135-173).
    fn light_cubes_changed(self, layer: core::ffi::c_int, xyz: &[i32], n: u32) -> Result<(), RenderError> {
        // SAFETY: live handle, `xyz` holds 3 * n coordinates and outlives the call
        self.check(unsafe {
            match self {
                Device::One(c) => ffi::aic_light_cubes_changed(c.as_ptr(), layer, n, xyz.as_ptr(), QUEUE_ORDER),
                Device::Many(m) => ffi::aic_multi_light_cubes_changed(m.as_ptr(), layer, n, xyz.as_ptr(), QUEUE_ORDER),
            }
        })
    }
    fn destroy(self) {
        // SAFETY: called once, from Drop
        unsafe {
            match self {
                Device::One(c) => ffi::aic_destroy(c.as_ptr()),
                Device::Many(m) => ffi::aic_destroy_multi(m.as_ptr()),
            }
        }
    }
}

/// hashbrown's `Group::WIDTH` on the host the reference's goldens came from: the order of equal-priority light updates
const QUEUE_ORDER: core::ffi::c_int = if cfg!(target_arch = "x86_64") { 16 } else { 8 };

/// The MI355X raytracer behind the reference's renderer interface.
pub struct HipRtRenderer {
    device: Device,
    cameras: StandardCameras,
    size_policy: Box<dyn Fn(Viewport) -> Viewport + Send + Sync>,
    layers: Layers<Option<LayerSync>>,
    had_cursor: bool,
    /// `Some(maximum_distance)`: the world layer's light is computed on the device (see `set_device_light`)
    device_light: Option<u8>,
    /// frames are bloomed on the device (`AIC_FRAME_BLOOM`, see `set_bloom`)
    bloom: bool,
    /// the context holds [`font_atlas`] (`aic_set_text_font`, on the first [`HipRtRenderer::present_split_text`])
    text_font_set: bool,
}

// SAFETY: the contexts are only used through `&mut self`; libaic_hip keeps no thread affinity besides hipSetDevice,
// which every entry point performs itself.
unsafe impl Send for HipRtRenderer {}

/// `impl Wireframe for Cursor` (all-is-cubes/src/character/cursor.rs:219-278) as the line list [`HipRtRenderer::present_split_lines`] draws: the hit
/// block's voxel bounds, the selected face's frame and the diamond at the point of entry, 12 to 28 lines in `palette::CURSOR_OUTLINE`. Host-only.
/// `None`: a face discriminant outside 0..=6, a resolution below 1 or a negative voxel size.
#[must_use]
pub fn cursor_wireframe(cursor: &ffi::aic_cursor_desc) -> Option<Vec<[ffi::aic_line_vertex; 2]>> {
    let mut out = vec![[ffi::aic_line_vertex::default(); 2]; ffi::AIC_CURSOR_MAX_LINES as usize];
    let mut n = 0u32;
    // SAFETY: `out` holds 2 * AIC_CURSOR_MAX_LINES vertices, the most the call writes
    let rc = unsafe { ffi::aic_cursor_wireframe(cursor, out.as_mut_ptr().cast(), &mut n) };
    if rc != 0 {
        return None;
    }
    out.truncate(n as usize);
    Some(out)
}

/// `impl Wireframe for LightUpdateCubeInfo` (all-is-cubes/src/space/light/debug.rs:50-95) as the line list [`HipRtRenderer::present_split_lines`]
/// draws, under `wireframe_vertices(v, Rgba::new(0.8, 0.8, 1.0, 1.0), ..)`: the cube's box, then per record its value cube's box and the arrow from the
/// cube's centre, coloured `light_from_struck_face`. `12 + 29 * rays.len()` lines. Host-only. `None`: `rays` is not the cube's `n_rays` records.
#[must_use]
pub fn light_rays_wireframe(info: &ffi::aic_light_cube_info, rays: &[ffi::aic_light_ray]) -> Option<Vec<[ffi::aic_line_vertex; 2]>> {
    if rays.len() != info.n_rays as usize {
        return None;
    }
    let mut out = vec![[ffi::aic_line_vertex::default(); 2]; 12 + 29 * rays.len()];
    let mut n = 0u32;
    // SAFETY: `out` holds 2 * (12 + 29 * n_rays) vertices, what the call writes; `rays` holds n_rays records
    let rc = unsafe { ffi::aic_light_rays_wireframe(info, rays.as_ptr(), out.as_mut_ptr().cast(), &mut n) };
    (rc == 0 && n as usize == out.len()).then_some(out)
}

/// `TerminalOptions` of the desktop program's terminal mode (all-is-cubes-desktop/src/terminal/options.rs:15-185), with the C ABI's values
/// (`ffi::AIC_CELLS_COLOR_*`, `ffi::AIC_CELLS_*`). The defaults are the reference's: `TwoFiftySix`, `Split`.
#[derive(Clone, Copy, Debug, Eq, Hash, PartialEq)]
pub struct TerminalOptions {
    pub colors: i32,
    pub characters: i32,
}

impl Default for TerminalOptions {
    fn default() -> Self {
        Self { colors: ffi::AIC_CELLS_COLOR_256, characters: ffi::AIC_CELLS_SPLIT }
    }
}

impl TerminalOptions {
    /// `ColorMode::cycle` (options.rs:61-68).
    pub fn cycle_colors(&mut self) {
        self.colors = (self.colors + 1) % 3;
    }

    /// `CharacterMode::cycle` (options.rs:166-175).
    pub fn cycle_characters(&mut self) {
        self.characters = (self.characters + 1) % 5;
    }

    /// `viewport_from_terminal_size` (options.rs:25-38; `aic_cells_geometry`): framebuffer width and height, nominal width and height. `None`: a
    /// dimension above 65535.
    #[must_use]
    pub fn viewport_from_terminal_size(&self, cols: u32, rows: u32) -> Option<([u32; 2], [f64; 2])> {
        let (mut w, mut h, mut nominal) = (0u32, 0u32, [0f64; 2]);
        // SAFETY: host-only; the three out-pointers are valid
        let rc = unsafe { ffi::aic_cells_geometry(cols, rows, self.characters, &mut w, &mut h, nominal.as_mut_ptr()) };
        (rc == 0).then_some(([w, h], nominal))
    }
}

/// `TerminalWindow::write_frame` (all-is-cubes-desktop/src/terminal/ui.rs:300-360; `aic_cells_ansi`) as a byte stream: `cells` is `[rows][cols]`,
/// `names[layer]` the text and column width of each block of that layer (a block beyond the table shows `#`), `origin` the corner of the rectangle to
/// draw into (`None`: rows end with a newline). Host-only. `None`: `cells` is not `cols * rows` long, or a name holds a NUL.
#[must_use]
pub fn cells_ansi(cells: &[ffi::aic_cell], cols: u32, rows: u32, names: [&[(&str, u8)]; 2], origin: Option<[u16; 2]>) -> Option<Vec<u8>> {
    if cells.len() != (cols as usize) * (rows as usize) {
        return None;
    }
    let mut strings: [Vec<std::ffi::CString>; 2] = [Vec::new(), Vec::new()];
    let mut pointers: [Vec<*const core::ffi::c_char>; 2] = [Vec::new(), Vec::new()];
    let mut widths: [Vec<u8>; 2] = [Vec::new(), Vec::new()];
    for layer in 0..2 {
        for (name, width) in names[layer] {
            strings[layer].push(std::ffi::CString::new(*name).ok()?);
            widths[layer].push(*width);
        }
        pointers[layer] = strings[layer].iter().map(|s| s.as_ptr()).collect();
    }
    let text = ffi::aic_cells_text {
        names: [pointers[0].as_ptr(), pointers[1].as_ptr()],
        widths: [widths[0].as_ptr(), widths[1].as_ptr()],
        n_names: [pointers[0].len() as u32, pointers[1].len() as u32],
        origin: origin.unwrap_or([0, 0]),
        reserved: 0,
    };
    let flags = if origin.is_some() { ffi::AIC_CELLS_ANSI_IN_RECT } else { 0 };
    let mut length = 0u64;
    // SAFETY: host-only; a capacity of 0 writes nothing and reports the length needed (the call's refusal of the capacity is expected)
    let _ = unsafe { ffi::aic_cells_ansi(cells.as_ptr(), cols, rows, &text, flags, core::ptr::null_mut(), 0, &mut length) };
    let mut out = vec![0u8; length as usize];
    // SAFETY: `out` holds `length` bytes, the tables outlive the call
    let rc = unsafe { ffi::aic_cells_ansi(cells.as_ptr(), cols, rows, &text, flags, out.as_mut_ptr().cast(), length, &mut length) };
    (rc == 0).then_some(out)
}

/// Cell width, height and margin of [`font_atlas`]: `FONT_SYSTEM_16`'s 7 x 16 character cell and an outline of one.
const FONT_CELL: [u32; 3] = [9, 18, 1];

/// The font atlas of the info text, as the reference makes it: `generate_texture_atlas` (all-is-cubes-gpu/src/text.rs:108-155) on
/// `Builtin::FontSystem16`. 16 x 16 cells of the character cell grown by an outline of one texel, RGBA8 with premultiplied alpha; each of the first
/// 256 scalar values drawn alone by `FontDef::draw_str_monospaced`, outline (0, 0, 0, 255), foreground (255, 255, 255, 255). Returns the texels,
/// row-major, and the cell's width, height and margin: what `aic_set_text_font` takes.
#[must_use]
pub fn font_atlas() -> (Vec<[u8; 4]>, [u32; 3]) {
    const OUTLINE_RADIUS: u32 = 1;
    let font = universe::Builtin::FontSystem16.read::<text::FontDef>();
    let logical = font.metrics().character_cell_size();
    let cell = [logical.width as u32 + 2 * OUTLINE_RADIUS, logical.height as u32 + 2 * OUTLINE_RADIUS];
    let row = 16 * cell[0] as usize;
    let mut atlas = vec![[0u8; 4]; row * 16 * cell[1] as usize];
    let mut buf = [0u8; 4];
    for code in 0u32..256 {
        let string = char::from_u32(code).expect("a scalar value below 256").encode_utf8(&mut buf);
        let origin = [(code % 16 * cell[0] + OUTLINE_RADIUS) as i32, (code / 16 * cell[1] + OUTLINE_RADIUS) as i32];
        font.draw_str_monospaced(string, |pixel, value| {
            let (x, y) = (pixel.x + origin[0], pixel.y + origin[1]);
            if x >= 0 && y >= 0 && (x as usize) < row && (y as usize) < 16 * cell[1] as usize {
                atlas[y as usize * row + x as usize] = match value {
                    text::Value::Outline => [0, 0, 0, 255],
                    text::Value::Foreground => [255, 255, 255, 255],
                };
            }
        });
    }
    (atlas, [cell[0], cell[1], OUTLINE_RADIUS])
}

fn options_of(o: &GraphicsOptions) -> ffi::aic_options {
    let (transparency, threshold) = match o.transparency {
        TransparencyOption::Surface => (0, 0.5),
        TransparencyOption::Volumetric => (1, 0.5),
        TransparencyOption::Threshold(t) => (2, t.into_inner()),
        _ => (1, 0.5),
    };
    let (lighting, bounce_samples) = match o.lighting_display {
        LightingOption::None => (0, 0),
        LightingOption::Flat => (1, 0),
        LightingOption::Coarse => (2, 0),
        LightingOption::Linear => (3, 0),
        LightingOption::Smoothstep => (4, 0),
        LightingOption::Bounce { samples } => (5, i32::from(samples)), // traced on the device (secondary rays inside the SHADE event)
        _ => (3, 0),
    };
    ffi::aic_options {
        fog: match o.fog { FogOption::None => 0, FogOption::Abrupt => 1, FogOption::Compromise => 2, FogOption::Physical => 3, _ => 1 },
        transparency,
        threshold,
        lighting,
        bounce_samples,
        antialiasing: match o.antialiasing { AntialiasingOption::None => 0, AntialiasingOption::IfCheap => 1, AntialiasingOption::Always => 2, _ => 0 },
        debug_pixel_cost: i32::from(o.debug_pixel_cost),
        tone_mapping: match o.tone_mapping { ToneMappingOperator::Clamp => 0, ToneMappingOperator::Reinhard => 1, _ => 0 },
        maximum_intensity: o.maximum_intensity.into_inner(),
        bloom_intensity: o.bloom_intensity.into_inner(),
        view_distance: o.view_distance.into_inner(),
    }
}

fn camera_of(camera: &Camera) -> ffi::aic_camera {
    ffi::aic_camera {
        // euclid's Transform3D::to_array is m11, m12, ..., m44: the order aic_camera documents
        inverse_projection_view: camera.inverse_projection_view().to_array(),
        exposure: camera.exposure().into_inner(),
        reserved: 0,
    }
}

impl HipRtRenderer {
    /// As `RtRenderer::new` (renderer.rs:65-81), on HIP device `device_id` (negative: the current device).
    ///
    /// # Errors
    /// Fails if no usable MI355X is present: there is no CPU fallback.
    pub fn new(
        cameras: StandardCameras,
        size_policy: Box<dyn Fn(Viewport) -> Viewport + Send + Sync>,
        device_id: i32,
    ) -> Result<Self, String> {
        Self::with_devices(cameras, size_policy, &[device_id])
    }

    /// One renderer over several GPUs of the node: the scene is replicated on each, every device traces its interleaved
    /// 8-row strips of a frame, the strips go to `device_ids[0]` over the direct links and are assembled there
    /// (`aic_create_multi`). With one id this is [`Self::new`].
    ///
    /// # Errors
    /// Fails if any of the devices is not a usable MI355X.
    pub fn with_devices(
        cameras: StandardCameras,
        size_policy: Box<dyn Fn(Viewport) -> Viewport + Send + Sync>,
        device_ids: &[i32],
    ) -> Result<Self, String> {
        // SAFETY: plain FFI calls; null returns are handled
        assert_eq!(unsafe { ffi::aic_abi_version() }, ffi::AIC_ABI_VERSION);
        let mut status = 0;
        let device = match device_ids {
            [] => return Err("no device given".into()),
            [one] => Device::One(
                NonNull::new(unsafe { ffi::aic_create(*one, &mut status) })
                    .ok_or_else(|| format!("aic_create failed with status {status} (no usable MI355X?)"))?,
            ),
            many => Device::Many(
                NonNull::new(unsafe { ffi::aic_create_multi(many.len() as core::ffi::c_int, many.as_ptr(), &mut status) })
                    .ok_or_else(|| format!("aic_create_multi failed with status {status}"))?,
            ),
        };
        Ok(Self { device, cameras, size_policy, layers: Layers::default(), had_cursor: false, device_light: None, bloom: false, text_font_set: false })
    }

    /// Blooms the frames drawn from now on as the reference's GPU renderer does (`AIC_FRAME_BLOOM`; all-is-cubes-gpu raytrace_to_texture.rs:644-661)
    /// whenever the world options' `bloom_intensity` is above zero; such a `Rendering` does not report `Flaws::NO_BLOOM`. Off by default.
    /// A multi-device renderer ignores it and keeps reporting `NO_BLOOM`.
    pub fn set_bloom(&mut self, on: bool) {
        self.bloom = on;
    }

    /// Whether frames are drawn with `AIC_FRAME_BLOOM`: [`Self::set_bloom`] on a single-device renderer (`aic_multi_render` has no bloom: device 0
    /// would first need every device's strips as ColorBufs).
    fn bloom_applies(&self) -> bool {
        self.bloom && matches!(self.device, Device::One(_))
    }

    /// Hands the world space's light over to the device: from now on `update` forwards block changes
    /// WITHOUT the host's light texels and queues the changed cubes in the device's own update queue
    /// (`LightStorage::modified_cube_needs_update`, updater.rs:135-173, as `aic_light_cubes_changed`), and
    /// [`Self::evaluate_light_budgeted`] advances the device's light between frames. The host `Space`'s light is
    /// neither read nor written. `None` returns to forwarding the host's light.
    pub fn set_device_light(&mut self, maximum_distance: Option<u8>) {
        self.device_light = maximum_distance;
    }

    fn sync_layer(
        device: Device,
        device_light: bool,
        layer: core::ffi::c_int,
        slot: &mut Option<LayerSync>,
        space: Option<&Handle<Space>>,
        read_ticket: ReadTicket<'_>,
        options: &GraphicsOptions,
    ) -> Result<(), RenderError> {
        // the Option-synchronisation of RtRenderer::update (renderer.rs:110-141)
        match (space, &mut *slot) {
            (Some(space), Some(sync)) if *space == sync.space => {}
            (Some(space), s) => {
                *s = Some(LayerSync {
                    space: space.clone(),
                    todo: listen::StoreLock::new(Todo { everything: true, ..Todo::default() }),
                    listening: false,
                    n_blocks: 0,
                    resent_blocks: Vec::new(),
                });
            }
            (None, s) => {
                if s.take().is_some() {
                    device.clear_space(layer)?;
                }
            }
        }
        let Some(sync) = slot else { return Ok(()) };
        let space = sync.space.read(read_ticket).map_err(RenderError::Read)?;
        if !sync.listening {
            space.listen(sync.todo.listener());
            sync.listening = true;
        }
        let todo = &mut *sync.todo.lock();
        let block_data = space.block_data();
        sync.resent_blocks.clear();
        if core::mem::take(&mut todo.everything) {
            // == SpaceRaytracer::new (sr.rs:64-88)
            let flat = FlatSpace::new(&space);
            device.upload_space(layer, &flat.desc())?;
            todo.blocks.clear();
            todo.cubes.clear();
        } else {
            // appended blocks, then re-evaluated ones (updating.rs:139-153): one batched call
            let mut indices: Vec<u32> = (sync.n_blocks..block_data.len()).map(|i| i as u32).collect();
            let appended = indices.len();
            indices.extend(todo.blocks.drain().map(u32::from).filter(|&i| (i as usize) < sync.n_blocks));
            sync.resent_blocks.extend_from_slice(&indices[appended..]);
            if !indices.is_empty() {
                let flat: Vec<_> = indices.iter().map(|&i| flatten_block(&block_data[i as usize])).collect();
                let descs: Vec<_> = flat.iter().map(|b| b.desc).collect();
                let voxels: Vec<_> = flat.iter().map(|b| b.voxels.as_ptr()).collect();
                let palettes: Vec<_> = flat.iter().map(|b| b.palette.as_ptr()).collect();
                device.replace_blocks(layer, &indices, &descs, &voxels, &palettes)?;
            }
            if !todo.cubes.is_empty() {
                let (xyz, idx, light) = gather_cubes(&space, todo.cubes.drain());
                if device_light && layer == ffi::AIC_LAYER_WORLD {
                    // block indices only; the device relights what changed. (A CubeLight message of the host Space lands
                    // here too and is harmless: the cube's block index is rewritten with the value it already has.)
                    device.update_cubes(layer, &xyz, &idx, None)?;
                    // (several devices: the updater runs on the first; `aic_multi_light_cubes_changed` scatters the texels it
                    //  wrote there into the others' volumes, so the next draw traces the same light on every device)
                    device.light_cubes_changed(layer, &xyz, idx.len() as u32)?;
                } else {
                    device.update_cubes(layer, &xyz, &idx, Some(&light))?;
                }
            }
        }
        sync.n_blocks = block_data.len();
        device.set_options(layer, &options_of(options))
    }

    /// `RtRenderer::update` (renderer.rs:96-141).
    pub fn update_scene(&mut self, read_tickets: Layers<ReadTicket<'_>>, cursor: Option<&Cursor>) -> Result<(), RenderError> {
        self.had_cursor = cursor.is_some();
        self.cameras.update(read_tickets);
        let (device, device_light) = (self.device, self.device_light.is_some());
        let world_options = self.cameras.graphics_options().clone();
        let ui_options = self.cameras.ui_view_state().graphics_options.clone();
        let world_space = self.cameras.world_space().get();
        Self::sync_layer(device, device_light, ffi::AIC_LAYER_WORLD, &mut self.layers.world, world_space.as_ref(), read_tickets.world, &world_options)?;
        let ui_space = self.cameras.ui_space().cloned();
        Self::sync_layer(device, device_light, ffi::AIC_LAYER_UI, &mut self.layers.ui, ui_space.as_ref(), read_tickets.ui, &ui_options)
    }

    /// The frame descriptor of the current cameras and the viewport it is drawn for.
    fn frame_desc(&self) -> (Viewport, ffi::aic_frame_desc) {
        let viewport = (self.size_policy)(self.cameras.viewport()); // renderer.rs:226-233
        let size = viewport.framebuffer_size;
        let backdrop = self.cameras.ui_view_state().backdrop;
        let frame = ffi::aic_frame_desc {
            width: size.width,
            height: size.height,
            world: camera_of(&self.cameras.cameras().world),
            ui: camera_of(&self.cameras.cameras().ui),
            backdrop: if backdrop == Rgba::TRANSPARENT {
                [0.0; 4]
            } else {
                [backdrop.red().into_inner(), backdrop.green().into_inner(), backdrop.blue().into_inner(), backdrop.alpha().into_inner()]
            },
            partition: ffi::aic_partition::default(),
            flags: if self.bloom_applies() { ffi::AIC_FRAME_BLOOM } else { 0 },
            tuning: 0, // the library's choices (tile queues, kernel variant); `HipInfo` reports what ran
        };
        (viewport, frame)
    }

    /// `RtRenderer::draw_rgba` (renderer.rs:282-308).
    pub fn draw_rgba(&mut self, info_text: &str) -> Result<Rendering, RenderError> {
        let (viewport, frame) = self.frame_desc();
        let size = viewport.framebuffer_size;
        let mut data = vec![[0u8; 4]; (size.width as usize) * (size.height as usize)];
        let mut info = ffi::aic_frame_info::default();
        if !data.is_empty() {
            // zero-area viewports produce an empty image (cases viewport_zero, cases/src/lib.rs:1167-1212)
            self.device.render(&frame, &mut data, &mut info)?;
        }
        self.wrap_rendering(viewport, data, info, info_text)
    }

    /// The frame as all-is-cubes-gpu's `raytrace_to_texture` stores it (raytrace_to_texture.rs:594-675): per pixel the `[f16; 4]` premultiplied colour
    /// times the exposure of the pixel's layer (as `f16` bits) and the `f32` projected depth of the nearest surface, negative on UI pixels -- the two
    /// texels of its `Split { color, depth, layer }` accumulator, written by the device (`AIC_FRAME_OUT_SPLIT`). The depth transform is that renderer's
    /// own (lines 613-618), taken from the world camera. No info text and no bloom: that renderer post-processes the colour target itself.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer (its strips are gathered as RGBA8).
    pub fn draw_split(&mut self) -> Result<(Vec<[u16; 4]>, Vec<f32>), RenderError> {
        let Device::One(ctx) = self.device else { panic!("draw_split needs a single-device renderer") };
        let (viewport, mut frame) = self.frame_desc();
        frame.flags = ffi::AIC_FRAME_OUT_SPLIT;
        let camera = &self.cameras.cameras().world;
        let depth_scale = -(camera.view_distance().into_inner() - camera.near_plane_distance().into_inner());
        let depth_bias = -camera.near_plane_distance().into_inner();
        let p = camera.projection_matrix();
        let zw = [depth_scale * p.m33, depth_bias * p.m33 + p.m43, depth_scale * p.m34, depth_bias * p.m34 + p.m44];
        // SAFETY: the context is live; `zw` holds the four coefficients the call copies
        self.device.check(unsafe { ffi::aic_set_depth_transform(ctx.as_ptr(), zw.as_ptr()) })?;
        let size = viewport.framebuffer_size;
        let n = (size.width as usize) * (size.height as usize);
        // one allocation of u64 words (the colour plane wants 8-byte texels): n of colour, then n / 2 rounded up of depth
        let mut planes = vec![0u64; n + n.div_ceil(2)];
        let mut info = ffi::aic_frame_info::default();
        if n != 0 {
            // SAFETY: the context is live; `planes` holds the 12 bytes per pixel the call writes and outlives it
            self.device.check(unsafe { ffi::aic_render(ctx.as_ptr(), &frame, planes.as_mut_ptr().cast(), 0, &mut info) })?;
        }
        let color = planes[..n].iter().map(|t| [*t as u16, (*t >> 16) as u16, (*t >> 32) as u16, (*t >> 48) as u16]).collect();
        let depth = (0..n).map(|i| f32::from_bits((planes[n + i / 2] >> (32 * (i % 2))) as u32)).collect();
        Ok((color, depth))
    }

    /// One frame of the terminal renderer (all-is-cubes-desktop/src/terminal.rs:119-137; `aic_render_cells`): the current viewport -- which must be
    /// [`TerminalOptions::viewport_from_terminal_size`] of `cols` x `rows` -- traced and turned into `[rows][cols]` character cells on the device.
    /// [`cells_ansi`] writes them out.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures, and when the viewport is not the grid's.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub fn draw_cells(&mut self, cols: u32, rows: u32, options: TerminalOptions) -> Result<(Vec<ffi::aic_cell>, ffi::aic_cells_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("draw_cells needs a single-device renderer") };
        let (_, frame) = self.frame_desc();
        let desc = ffi::aic_cells_desc { cols, rows, characters: options.characters, colors: options.colors, ..Default::default() };
        let mut cells = vec![ffi::aic_cell::default(); (cols.max(1) as usize) * (rows.max(1) as usize)];
        let mut frame_info = ffi::aic_frame_info::default();
        let mut cells_info = ffi::aic_cells_info::default();
        // SAFETY: the context is live; `cells` holds the raised grid the call writes and outlives it
        self.device.check(unsafe { ffi::aic_render_cells(ctx.as_ptr(), &frame, &desc, cells.as_mut_ptr(), 0, &mut frame_info, &mut cells_info) })?;
        Ok((cells, cells_info))
    }

    /// `image_patch_to_character` (terminal/chars.rs:18-173; `aic_image_cells`) for every cell of an image in device memory, e.g. the f16 presentation
    /// of a resident Split frame (`flags`: `AIC_CELLS_IMAGE_DEVICE | AIC_CELLS_IMAGE_F16 | AIC_CELLS_POSTPROCESSED`).
    ///
    /// # Safety
    /// `image_device` (and `aux_device`, unless null) must hold the framebuffer of `desc` on the renderer's device, laid out as `desc.flags` says.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures and rejected arguments.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub unsafe fn image_cells_device(&mut self, desc: &ffi::aic_cells_desc, image_device: *const core::ffi::c_void, aux_device: *const ffi::aic_pixel_aux) -> Result<(Vec<ffi::aic_cell>, ffi::aic_cells_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("image_cells_device needs a single-device renderer") };
        let mut desc = *desc;
        desc.flags = (desc.flags | ffi::AIC_CELLS_IMAGE_DEVICE) & !ffi::AIC_CELLS_OUT_DEVICE;
        let mut cells = vec![ffi::aic_cell::default(); (desc.cols.max(1) as usize) * (desc.rows.max(1) as usize)];
        let mut info = ffi::aic_cells_info::default();
        // SAFETY: the context is live; the caller vouches for the device pointers; `cells` holds the raised grid
        self.device.check(unsafe { ffi::aic_image_cells(ctx.as_ptr(), &desc, image_device, aux_device, cells.as_mut_ptr(), &mut info) })?;
        Ok((cells, info))
    }

    /// The finished pixels as the trait's `Rendering`: info text, flaws, info.
    fn wrap_rendering(&self, viewport: Viewport, mut data: Vec<[u8; 4]>, info: ffi::aic_frame_info, info_text: &str) -> Result<Rendering, RenderError> {
        let size = viewport.framebuffer_size;
        let options = self.cameras.graphics_options();
        if options.debug_info_text && !info_text.is_empty() && !data.is_empty() {
            // renderer.rs:205-217: the encoder's black and white (exposure and tone mapping applied, as the kernel's encoder does)
            let camera = &self.cameras.cameras().world;
            let paint = [
                camera.post_process_color(Rgba::BLACK).to_srgb8(),
                camera.post_process_color(Rgba::WHITE).to_srgb8(),
            ];
            draw_info_text(&mut data, viewport, &paint, info_text);
        }
        let mut flaws = Flaws::empty();
        if info.flaws & ffi::AIC_FLAW_UNSUPPORTED != 0 {
            flaws |= Flaws::UNSUPPORTED;
        }
        if options.bloom_intensity != ZeroOne::ZERO && !self.bloom_applies() {
            flaws |= Flaws::NO_BLOOM; // renderer.rs:293-297 (a bloomed frame has what the reference's GPU renderer adds)
        }
        if self.had_cursor {
            flaws |= Flaws::NO_CURSOR; // renderer.rs:298-300
        }
        Ok(Rendering { size, data, flaws, info: Arc::new(HipInfo(info)) })
    }

    /// Queues the current view on `slot` (0..`AIC_MULTI_MAX_IN_FLIGHT`) and returns at once: the streaming half of `draw_rgba` for a caller that renders
    /// frame after frame (record.rs:97-113 steps the universe, updates and draws in a loop) -- `update_scene` for frame n + 1 and its `begin_frame` may run
    /// while frame n is still being traced and assembled. On a multi-device renderer this is `aic_multi_render_submit`; a single-device renderer has no
    /// host-target streaming entry point (`aic_render_submit` writes device memory), so the frame is drawn here and merely handed over by `finish_frame`.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures; a busy slot is an error.
    pub fn begin_frame(&mut self, slot: u32) -> Result<PendingFrame, RenderError> {
        let (viewport, frame) = self.frame_desc();
        let size = viewport.framebuffer_size;
        let mut data = vec![[0u8; 4]; (size.width as usize) * (size.height as usize)];
        let mut info = ffi::aic_frame_info::default();
        let streamed = match self.device {
            // SAFETY: live handle; `data`'s heap buffer is not moved or freed before `finish_frame` (PendingFrame owns it), and holds width * height pixels
            Device::Many(m) if !data.is_empty() => {
                self.device.check(unsafe { ffi::aic_multi_render_submit(m.as_ptr(), &frame, data.as_mut_ptr().cast(), 0, slot) })?;
                true
            }
            _ => {
                if !data.is_empty() {
                    self.device.render(&frame, &mut data, &mut info)?;
                }
                false
            }
        };
        Ok(PendingFrame { slot, streamed, viewport, data, info })
    }

    /// Waits for the frame `begin_frame` queued and wraps it as `draw_rgba` would.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    pub fn finish_frame(&mut self, mut pending: PendingFrame, info_text: &str) -> Result<Rendering, RenderError> {
        if pending.streamed {
            if let Device::Many(m) = self.device {
                // SAFETY: live handle, `info` is a valid out-pointer; the library writes `pending.data` before this returns
                self.device.check(unsafe { ffi::aic_multi_render_wait(m.as_ptr(), pending.slot, &mut pending.info) })?;
            }
        }
        self.wrap_rendering(pending.viewport, pending.data, pending.info, info_text)
    }

    /// The cameras this renderer draws (as `RtRenderer::cameras`).
    pub fn cameras(&self) -> &StandardCameras {
        &self.cameras
    }

    /// `SpaceRaytracer::trace_ray(ray, accumulator, include_sky)` (sr.rs:113-120) for a batch of world-space rays against the
    /// space of `layer` (`ffi::AIC_LAYER_WORLD` / `ffi::AIC_LAYER_UI`) as last uploaded by `update`: no camera, no layering, one
    /// ray per result. `rays[i]` = origin x, y, z, direction x, y, z; a direction is taken as given, not normalised. Returns,
    /// per ray, the `ColorBuf` `trace_ray` leaves in its accumulator (light r, g, b and transmittance) and the first-hit
    /// record (`hit == 0`: none; `t_distance` in units of the direction).
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer (ray batches are not sharded), a layer without a space, or more than 2048 x 65535 rays.
    pub fn trace_rays(&mut self, layer: core::ffi::c_int, rays: &[[f64; 6]], include_sky: bool) -> Result<(Vec<[f32; 4]>, Vec<ffi::aic_pixel_aux>), RenderError> {
        let Device::One(ctx) = self.device else { panic!("trace_rays needs a single-device renderer") };
        let n = u32::try_from(rays.len()).expect("more than u32::MAX rays");
        let mut colors = vec![[0.0f32; 4]; rays.len()];
        let mut hits = vec![ffi::aic_pixel_aux::default(); rays.len()];
        let mut info = ffi::aic_frame_info::default();
        let flags = ffi::AIC_FRAME_OUT_COLORBUF | if include_sky { 0 } else { ffi::AIC_RAYS_NO_SKY };
        // SAFETY: the context is live; the three buffers hold `n` elements each and outlive the call, which returns when the batch is done
        self.device.check(unsafe {
            ffi::aic_trace_rays(ctx.as_ptr(), layer, n, rays.as_ptr().cast(), flags, 1.0, colors.as_mut_ptr().cast(), hits.as_mut_ptr(), &mut info)
        })?;
        Ok((colors, hits))
    }

    /// The sampling loop of `character::exposure::State::step` (exposure.rs:91-128) for a batch of world-space rays against the space of `layer` as
    /// last uploaded by `update`, with its light wherever it was made: per ray the luminance of the light behind the first visible block that has a
    /// valid one, or of the sky. `max_steps` is `2 * maximum_distance`, 0 for `LightPhysics::None`. Legal while frames are in flight. A multi-device
    /// renderer samples on its first device: the scene is replicated.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a layer without a space, or more than `1 << 20` rays.
    pub fn sample_luminance(&mut self, layer: core::ffi::c_int, rays: &[[f64; 6]], max_steps: u32) -> Result<Vec<f32>, RenderError> {
        let n = u32::try_from(rays.len()).expect("more than u32::MAX rays");
        let mut out = vec![0.0f32; rays.len()];
        // SAFETY: the context is live; both buffers hold `n` elements and outlive the call, which returns when the samples are there
        self.device.check(unsafe { ffi::aic_sample_luminance(self.device.first_ctx(), layer, n, rays.as_ptr().cast(), max_steps, 0, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// `cursor_raycast` (all-is-cubes/src/character/cursor.rs:26-107) for a batch of rays against the space of `layer` as last uploaded by `update`,
    /// on the device: per ray the first selectable block struck within `maximum_distance` (infinity is legal), or `None`. The record is what a
    /// `Cursor` holds that the device knows -- `Cursor`'s own fields are private to its crate and its `hit().block` / `evaluated` are objects of the
    /// application's, found through `block_index` -- and its `cursor` member is what [`cursor_wireframe`] takes. Legal while frames are in flight.
    /// A multi-device renderer raycasts on its first device: the scene is replicated.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a layer without a space, a NaN or negative `maximum_distance`, or more than `1 << 20` rays.
    pub fn cursor_raycast(&mut self, layer: core::ffi::c_int, rays: &[[f64; 6]], maximum_distance: f64) -> Result<Vec<Option<ffi::aic_cursor_hit>>, RenderError> {
        let n = u32::try_from(rays.len()).expect("more than u32::MAX rays");
        let mut out = vec![ffi::aic_cursor_hit::default(); rays.len()];
        // SAFETY: the context is live; both buffers hold `n` elements and outlive the call, which returns when the records are there
        self.device.check(unsafe { ffi::aic_cursor_raycast(self.device.first_ctx(), layer, n, rays.as_ptr().cast(), maximum_distance, 0, out.as_mut_ptr()) })?;
        Ok(out.into_iter().map(|h| (h.hit != 0).then_some(h)).collect())
    }

    /// `Space::compute_light::<LightUpdateCubeInfo>` (all-is-cubes/src/space/light/updater.rs:368-417, light/debug.rs) for a batch of cubes against
    /// the published light volume of `layer`, on the device: what `GraphicsOptions::debug_light_rays_at_cursor` draws for `cursor.preceding_cube()`.
    /// Per cube its info (the texel and cost `compute_light` returns, its number of records) and its records in the order the reference pushes them;
    /// everything the batch produces is returned. [`light_rays_wireframe`] turns one cube's answer into lines. Legal while frames are in flight. A
    /// multi-device renderer asks its first device: the scene and the light are replicated.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a layer without a space, or more than `1 << 16` cubes.
    pub fn light_rays(&mut self, layer: core::ffi::c_int, cubes: &[[i32; 3]], maximum_distance: u8) -> Result<Vec<(ffi::aic_light_cube_info, Vec<ffi::aic_light_ray>)>, RenderError> {
        let n = u32::try_from(cubes.len()).expect("more than u32::MAX cubes");
        // SAFETY: host-only, no pointers
        let bound = unsafe { ffi::aic_light_rays_bound(i32::from(maximum_distance)) };
        let capacity = n.checked_mul(bound).expect("more records than u32::MAX");
        let mut infos = vec![ffi::aic_light_cube_info::default(); cubes.len()];
        let mut rays = vec![ffi::aic_light_ray::default(); capacity as usize];
        let mut totals = [0u64; 2];
        // SAFETY: the context is live; `infos` holds `n` records and `rays` `capacity`, both outlive the call, which returns when the records are there
        self.device.check(unsafe {
            ffi::aic_light_rays(self.device.first_ctx(), layer, n, cubes.as_ptr().cast(), i32::from(maximum_distance), 0, capacity, infos.as_mut_ptr(), rays.as_mut_ptr(), core::ptr::null_mut(), totals.as_mut_ptr())
        })?;
        Ok(infos.into_iter().map(|i| (i, rays[i.first_ray as usize..(i.first_ray + i.n_rays) as usize].to_vec())).collect())
    }

    /// `StandardCameras::project_cursor` (all-is-cubes-render/src/camera/stdcam.rs:357-389) through the cameras of the last `update`: the UI space,
    /// if there is one, at any distance; else, or if nothing is struck there, the character's space at 6.0.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    pub fn project_cursor(&mut self, ndc_pos: all_is_cubes_render::camera::NdcPoint2) -> Result<Option<ffi::aic_cursor_hit>, RenderError> {
        let ray_of = |ray: all_is_cubes::raycast::Ray| [ray.origin.x, ray.origin.y, ray.origin.z, ray.direction.x, ray.direction.y, ray.direction.z];
        if self.cameras.ui_space().is_some() {
            let ray = ray_of(self.cameras.cameras().ui.project_ndc_into_world(ndc_pos));
            if let Some(hit) = self.cursor_raycast(ffi::AIC_LAYER_UI, &[ray], f64::INFINITY)?.pop().flatten() {
                return Ok(Some(hit));
            }
        }
        if self.cameras.character().is_some() && self.cameras.world_space().get().is_some() {
            let ray = ray_of(self.cameras.cameras().world.project_ndc_into_world(ndc_pos));
            // TODO: maximum distance should be determined by character/universe parameters instead of hardcoded
            if let Some(hit) = self.cursor_raycast(ffi::AIC_LAYER_WORLD, &[ray], 6.0)?.pop().flatten() {
                return Ok(Some(hit));
            }
        }
        Ok(None)
    }

    /// One round of `raytrace_to_texture`'s `do_some_tracing` (raytrace_to_texture.rs:591-751): the listed pixels (`y * width + x`) of the frame
    /// `draw_split` renders, each traced exactly as there (`RtScene::trace_patch` on the pixel's own rectangle). Returns the two texels per pixel in list
    /// order -- the f16 colour bits and the signed depth -- for the caller to write at those pixels of its resident textures. A pixel may be listed more
    /// than once, as [`PixelPicker`]'s inner cycle does.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures; a listed pixel outside the viewport is an error.
    ///
    /// # Panics
    /// On a multi-device renderer, or more than 2048 x 65535 pixels.
    pub fn trace_pixels(&mut self, pixels: &[u32]) -> Result<(Vec<[u16; 4]>, Vec<f32>), RenderError> {
        let Device::One(ctx) = self.device else { panic!("trace_pixels needs a single-device renderer") };
        let (_, mut frame) = self.frame_desc();
        frame.flags = ffi::AIC_FRAME_OUT_SPLIT;
        let camera = &self.cameras.cameras().world;
        let depth_scale = -(camera.view_distance().into_inner() - camera.near_plane_distance().into_inner());
        let depth_bias = -camera.near_plane_distance().into_inner();
        let p = camera.projection_matrix();
        let zw = [depth_scale * p.m33, depth_bias * p.m33 + p.m43, depth_scale * p.m34, depth_bias * p.m34 + p.m44];
        // SAFETY: the context is live; `zw` holds the four coefficients the call copies
        self.device.check(unsafe { ffi::aic_set_depth_transform(ctx.as_ptr(), zw.as_ptr()) })?;
        let n = pixels.len();
        let n32 = u32::try_from(n).expect("more than u32::MAX pixels");
        // one allocation of u64 words, as in draw_split: n of colour, then n / 2 rounded up of depth
        let mut planes = vec![0u64; n + n.div_ceil(2)];
        let mut info = ffi::aic_frame_info::default();
        // SAFETY: the context is live; `pixels` holds n indices, `planes` the 12 bytes per pixel the call writes; the call returns when the batch is done
        self.device.check(unsafe {
            ffi::aic_trace_pixels(ctx.as_ptr(), &frame, n32, pixels.as_ptr(), 0, planes.as_mut_ptr().cast(), core::ptr::null_mut(), &mut info)
        })?;
        let color = planes[..n].iter().map(|t| [*t as u16, (*t >> 16) as u16, (*t >> 32) as u16, (*t >> 48) as u16]).collect();
        let depth = (0..n).map(|i| f32::from_bits((planes[n + i / 2] >> (32 * (i % 2))) as u32)).collect();
        Ok((color, depth))
    }

    /// `raytrace_to_texture`'s `prepare_frame` when the camera has moved since its textures were traced (raytrace_to_texture.rs:433-540): the resident
    /// Split frame at `src_device`, traced with `traced_with`, is drawn into the current world camera as depth-tested point sprites
    /// (`rt_reproject_vertex` / `rt_reproject_fragment`) and gap-filled (`gap_fill_downsample` / `gap_fill_upsample`), into `dst_device` -- again a
    /// resident Split frame (colour plane, then the depth plane at byte offset `width * height * 8`), which a round of tracing refines in place.
    /// `flags`: `ffi::AIC_REPROJECT_*`.
    ///
    /// # Safety
    /// `src_device` and `dst_device` are device memory on the renderer's device, each `width * height * 12` bytes of the current viewport, 8-byte
    /// aligned and not overlapping.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub unsafe fn reproject_split(
        &mut self,
        src_device: *const core::ffi::c_void,
        dst_device: *mut core::ffi::c_void,
        traced_with: &Camera,
        flags: u32,
    ) -> Result<ffi::aic_reproject_info, RenderError> {
        let Device::One(ctx) = self.device else { panic!("reproject_split needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        // raytrace_to_texture.rs:446-453, and camera::convert_matrix: euclid's rows become WGSL's columns
        let m = traced_with
            .view_matrix()
            .then(&traced_with.projection_matrix())
            .inverse()
            .unwrap_or_default()
            .then(&camera.view_matrix())
            .then(&camera.projection_matrix());
        let ip = camera.projection_matrix().inverse().unwrap_or_default();
        let desc = ffi::aic_reproject_desc {
            width: viewport.framebuffer_size.width,
            height: viewport.framebuffer_size.height,
            reprojection: m.to_array().map(|v| v as f32),
            inverse_projection_zw: [ip.m33 as f32, ip.m43 as f32, ip.m34 as f32, ip.m44 as f32],
            flags,
            reserved: 0,
        };
        let mut info = ffi::aic_reproject_info::default();
        // SAFETY: the context is live; the caller vouches for the two frames; the call returns when dst is written
        self.device.check(unsafe { ffi::aic_reproject_split(ctx.as_ptr(), &desc, src_device, dst_device, &mut info) })?;
        Ok(info)
    }

    /// `PixelPicker::take` on the device (raytrace_to_texture.rs:838-908): the next `n` pixel indices of the renderer's viewport written to
    /// `pixels_out_device`, ready for `aic_trace_pixels` with `AIC_PIXELS_DEVICE | AIC_PIXELS_IN_PLACE`. With `max_unknown > 0` the list begins with up
    /// to that many of the pixels the last [`Self::reproject_split`] knows nothing about, in picker order, skipping the first `skip_unknown` of them
    /// (those already handed out); the rest is the reference's pick sequence from pick index `cursor`. The caller keeps `cursor` (the info's
    /// `next_cursor`) and `skip_unknown` (add `n_from_unknown`; zero after a reprojection).
    ///
    /// # Safety
    /// `order_device` is null (row-major) or `width * height` `u32` of device memory on the renderer's device holding `aic_pixel_order`'s result for the
    /// current viewport; `pixels_out_device` is `n` `u32` of device memory there; both 4-byte aligned.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures; `max_unknown > 0` without a reprojection of the current viewport's size behind it is rejected.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub unsafe fn pick_pixels(
        &mut self,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        n: u32,
        max_unknown: u32,
        skip_unknown: u64,
        cursor: u64,
    ) -> Result<ffi::aic_pick_info, RenderError> {
        let Device::One(ctx) = self.device else { panic!("pick_pixels needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let desc = ffi::aic_pick_desc {
            width: viewport.framebuffer_size.width,
            height: viewport.framebuffer_size.height,
            n,
            max_unknown,
            skip_unknown,
            cursor,
            flags: 0,
            reserved: 0,
        };
        let mut info = ffi::aic_pick_info::default();
        // SAFETY: the context is live; the caller vouches for the two lists; the call returns when the list is written
        self.device.check(unsafe { ffi::aic_pick_pixels(ctx.as_ptr(), &desc, order_device, pixels_out_device, &mut info) })?;
        Ok(info)
    }

    /// The screen rectangles of the pixels that boxes of changed cubes can have changed under the renderer's current world camera (`aic_stale_rects`):
    /// one rectangle per box `[lower, upper)` grown by `expand` cubes -- 1 covers the light stencil and ambient occlusion beside a changed cube.
    /// Host-only. `None`: a negative `expand` or a viewport edge above 65535.
    pub fn stale_rects(&self, boxes: &[[i32; 6]], expand: i32) -> Option<Vec<ffi::aic_stale_rect>> {
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        let view_projection: [f64; 16] = camera.view_matrix().then(&camera.projection_matrix()).to_array();
        let mut out = vec![ffi::aic_stale_rect::default(); boxes.len()];
        let n = u32::try_from(boxes.len()).ok()?;
        // SAFETY: both lists hold `n` records; the matrix is 16 doubles
        let rc = unsafe {
            ffi::aic_stale_rects(
                view_projection.as_ptr(),
                viewport.framebuffer_size.width,
                viewport.framebuffer_size.height,
                n,
                boxes.as_ptr().cast(),
                expand,
                out.as_mut_ptr(),
            )
        };
        (rc == 0).then_some(out)
    }

    /// [`Self::pick_pixels`] with the pixels a scene change made stale first (`aic_pick_stale`; not in the reference, which re-arms a whole picker
    /// cycle, raytrace_to_texture.rs:587-589): the list begins with up to `max_stale` of the pixels of the resident Split frame at `src_device` that lie
    /// inside one of `rects` ([`Self::stale_rects`]) which does not keep them out, in picker order, skipping the first `skip_stale`; the rest is the
    /// reference's pick sequence from `cursor`. With `ffi::AIC_STALE_DEPTH_TEST` in `flags` a rectangle keeps out an opaque world pixel in front of
    /// its box; without it the frame is not read. The caller keeps `cursor` and `skip_stale` (add `n_from_stale`; zero with new rectangles).
    ///
    /// # Safety
    /// As [`Self::pick_pixels`]; `src_device` is a whole Split frame of the current viewport on the renderer's device, 8-byte aligned (it may be null
    /// without the depth test).
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures; more than `ffi::AIC_STALE_MAX_RECTS` rectangles are rejected.
    ///
    /// # Panics
    /// On a multi-device renderer.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn pick_stale(
        &mut self,
        rects: &[ffi::aic_stale_rect],
        flags: u32,
        src_device: *const core::ffi::c_void,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        n: u32,
        max_stale: u32,
        skip_stale: u64,
        cursor: u64,
    ) -> Result<ffi::aic_stale_info, RenderError> {
        let Device::One(ctx) = self.device else { panic!("pick_stale needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let desc = ffi::aic_stale_desc {
            width: viewport.framebuffer_size.width,
            height: viewport.framebuffer_size.height,
            n,
            max_stale,
            skip_stale,
            cursor,
            n_rects: u32::try_from(rects.len()).unwrap_or(u32::MAX),
            flags,
            rects: rects.as_ptr(),
        };
        let mut info = ffi::aic_stale_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the two lists; `rects` is copied before the call returns
        self.device.check(unsafe { ffi::aic_pick_stale(ctx.as_ptr(), &desc, src_device, order_device, pixels_out_device, &mut info) })?;
        Ok(info)
    }

    /// The cubes of the world layer whose light texel the light updater changed since the last take (`aic_light_changed_take`; not in the reference):
    /// what [`Self::pick_stale_cubes`] takes as `light_cubes`. Exact, ascending in the volume's cube index; the caller's own light writes are never
    /// reported. A submitted light update is ended and published first.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub fn take_changed_light_cubes(&mut self) -> Result<Vec<[i32; 3]>, RenderError> {
        let Device::One(ctx) = self.device else { panic!("take_changed_light_cubes needs a single-device renderer") };
        let mut written = 0u32;
        // SAFETY: the context is live; a take of no capacity writes no cube -- it ends a submitted update, and succeeds only when nothing is reported
        if unsafe { ffi::aic_light_changed_take(ctx.as_ptr(), ffi::AIC_LAYER_WORLD, 0, core::ptr::null_mut(), &mut written) } == 0 {
            return Ok(Vec::new());
        }
        let mut n = 0u64;
        // SAFETY: the context is live; bounds may be null
        self.device.check(unsafe { ffi::aic_light_changed_count(ctx.as_ptr(), ffi::AIC_LAYER_WORLD, &mut n, core::ptr::null_mut()) })?;
        let mut out = vec![[0i32; 3]; usize::try_from(n).unwrap_or(usize::MAX)];
        // SAFETY: `out` holds `n` cubes of three coordinates
        self.device.check(unsafe {
            ffi::aic_light_changed_take(ctx.as_ptr(), ffi::AIC_LAYER_WORLD, u32::try_from(n).unwrap_or(u32::MAX), out.as_mut_ptr().cast(), &mut written)
        })?;
        out.truncate(written as usize);
        Ok(out)
    }

    /// [`Self::pick_stale`] from the changed cubes themselves, any number of them (`aic_pick_stale_cubes`; not in the reference): `boxes` are changed
    /// blocks `[lower, upper)`, grown by `expand` as under [`Self::stale_rects`]; `light_cubes` are cubes whose light texel changed
    /// ([`Self::take_changed_light_cubes`]), each the box `[q, q + 1)` grown by one. The device projects them under the renderer's current world
    /// camera and marks their rectangles, so the cost follows the rectangles' area. `ffi::AIC_STALE_DEPTH_TEST` is [`Self::pick_stale`]'s front test;
    /// with `ffi::AIC_STALE_DEPTH_BEHIND` a light cube's rectangle keeps out a world pixel whose depth lies beyond the cube's greatest depth, which is
    /// exact under translucency and antialiasing (the depth texel is the nearest surface's).
    ///
    /// # Safety
    /// As [`Self::pick_stale`].
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn pick_stale_cubes(
        &mut self,
        boxes: &[[i32; 6]],
        expand: i32,
        light_cubes: &[[i32; 3]],
        flags: u32,
        src_device: *const core::ffi::c_void,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        n: u32,
        max_stale: u32,
        skip_stale: u64,
        cursor: u64,
    ) -> Result<ffi::aic_stale_cubes_info, RenderError> {
        let Device::One(ctx) = self.device else { panic!("pick_stale_cubes needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        let desc = ffi::aic_stale_cubes_desc {
            width: viewport.framebuffer_size.width,
            height: viewport.framebuffer_size.height,
            n,
            max_stale,
            skip_stale,
            cursor,
            view_projection: camera.view_matrix().then(&camera.projection_matrix()).to_array(),
            n_boxes: u32::try_from(boxes.len()).unwrap_or(u32::MAX),
            expand,
            n_light_cubes: u32::try_from(light_cubes.len()).unwrap_or(u32::MAX),
            flags,
            boxes: boxes.as_ptr().cast(),
            light_cubes: light_cubes.as_ptr().cast(),
        };
        let mut info = ffi::aic_stale_cubes_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the two lists; both arrays are copied before the call returns
        self.device.check(unsafe { ffi::aic_pick_stale_cubes(ctx.as_ptr(), &desc, src_device, order_device, pixels_out_device, &mut info) })?;
        Ok(info)
    }

    /// The world layer's block indices whose definition the last [`Self::update_scene`] re-sent (the reference's `todo.blocks`, updating.rs:139-153):
    /// the cube grid did not change under them, only what the cubes holding them look like. [`Self::pick_stale_blocks`] takes them as `blocks`.
    /// Empty after a whole upload, which makes every pixel stale.
    #[must_use]
    pub fn changed_blocks(&self) -> &[u32] {
        self.layers.world.as_ref().map_or(&[][..], |sync| sync.resent_blocks.as_slice())
    }

    /// The cubes of the world layer that hold one of the block indices `blocks`, as runs along z (`aic_find_block_cubes`; not in the reference): boxes
    /// `[lower, upper)` sorted by a run's first cube in the grid's linear order. With more runs than `capacity` the one box `info.bounds` is returned
    /// instead (none with `capacity` 0) and `info.merged` is 1.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub fn find_block_cubes(&mut self, blocks: &[u32], capacity: u32) -> Result<(Vec<[i32; 6]>, ffi::aic_block_cubes_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("find_block_cubes needs a single-device renderer") };
        let mut out = vec![[0i32; 6]; capacity as usize];
        let mut info = ffi::aic_block_cubes_info::default();
        // SAFETY: the context is live; `blocks` holds as many indices as are passed and `out` holds `capacity` boxes of six coordinates
        self.device.check(unsafe {
            ffi::aic_find_block_cubes(
                ctx.as_ptr(),
                ffi::AIC_LAYER_WORLD,
                u32::try_from(blocks.len()).unwrap_or(u32::MAX),
                blocks.as_ptr(),
                capacity,
                if capacity == 0 { core::ptr::null_mut() } else { out.as_mut_ptr().cast() },
                &mut info,
            )
        })?;
        out.truncate(info.n_written as usize);
        Ok((out, info))
    }

    /// The block index of every cube of the world layer from `block_index_device` (and the light from `light_device`, unless null), arrays in device
    /// memory on the renderer's device (`aic_replace_cube_grid`; not in the reference): a world made on the device becomes the scene without a trip
    /// through the host. Returns the runs of changed cubes along z as boxes `[lower, upper)`, as [`Self::find_block_cubes`] gives them -- with more
    /// runs than `capacity` the one box `info.bounds` --, ready for [`Self::pick_stale_cubes`]. The `Space` the renderer listens to is not told.
    ///
    /// # Safety
    /// `block_index_device` points to one `u16` per cube of the world space, 16-byte aligned, and `light_device` is null or points to four bytes per
    /// cube, both in device memory and complete (their stream synchronised).
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures; an index at or above the block count is refused with the scene untouched.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub unsafe fn replace_cube_grid_device(
        &mut self,
        block_index_device: *const u16,
        light_device: *const u8,
        capacity: u32,
    ) -> Result<(Vec<[i32; 6]>, ffi::aic_block_cubes_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("replace_cube_grid_device needs a single-device renderer") };
        let mut out = vec![[0i32; 6]; capacity as usize];
        let mut info = ffi::aic_block_cubes_info::default();
        // SAFETY: the context is live; the caller vouches for the device arrays and `out` holds `capacity` boxes of six coordinates
        self.device.check(unsafe {
            ffi::aic_replace_cube_grid(
                ctx.as_ptr(),
                ffi::AIC_LAYER_WORLD,
                block_index_device,
                light_device,
                capacity,
                if capacity == 0 { core::ptr::null_mut() } else { out.as_mut_ptr().cast() },
                &mut info,
            )
        })?;
        out.truncate(info.n_written as usize);
        Ok((out, info))
    }

    /// [`Self::pick_stale_cubes`] with, behind `boxes`, the boxes [`Self::find_block_cubes`]`(blocks, max_runs)` gives, found and kept on the device
    /// (`aic_pick_stale_blocks`; not in the reference): the pixels a re-evaluated block made stale first. `blocks` is [`Self::changed_blocks`] of the
    /// update that re-sent them, kept by the caller until no stale pixel is handed out any more.
    ///
    /// # Safety
    /// As [`Self::pick_stale`].
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn pick_stale_blocks(
        &mut self,
        boxes: &[[i32; 6]],
        expand: i32,
        light_cubes: &[[i32; 3]],
        blocks: &[u32],
        max_runs: u32,
        flags: u32,
        src_device: *const core::ffi::c_void,
        order_device: *const u32,
        pixels_out_device: *mut u32,
        n: u32,
        max_stale: u32,
        skip_stale: u64,
        cursor: u64,
    ) -> Result<ffi::aic_stale_blocks_info, RenderError> {
        let Device::One(ctx) = self.device else { panic!("pick_stale_blocks needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        let desc = ffi::aic_stale_blocks_desc {
            cubes: ffi::aic_stale_cubes_desc {
                width: viewport.framebuffer_size.width,
                height: viewport.framebuffer_size.height,
                n,
                max_stale,
                skip_stale,
                cursor,
                view_projection: camera.view_matrix().then(&camera.projection_matrix()).to_array(),
                n_boxes: u32::try_from(boxes.len()).unwrap_or(u32::MAX),
                expand,
                n_light_cubes: u32::try_from(light_cubes.len()).unwrap_or(u32::MAX),
                flags,
                boxes: boxes.as_ptr().cast(),
                light_cubes: light_cubes.as_ptr().cast(),
            },
            layer: ffi::AIC_LAYER_WORLD,
            n_blocks: u32::try_from(blocks.len()).unwrap_or(u32::MAX),
            block_indices: blocks.as_ptr(),
            max_runs,
            reserved: 0,
        };
        let mut info = ffi::aic_stale_blocks_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the two lists; the three arrays are copied before the call returns
        self.device.check(unsafe { ffi::aic_pick_stale_blocks(ctx.as_ptr(), &desc, src_device, order_device, pixels_out_device, &mut info) })?;
        Ok(info)
    }

    /// What `raytrace_to_texture` does with its resident textures every displayed frame (raytrace_to_texture.rs:546-568, shaders/rt-copy.wgsl:41-71,
    /// bloom.rs:41-60, shaders/postprocess.wgsl:140-158 and 251-276): the resident Split frame at `src_device`, of the renderer's own viewport, is
    /// stretched with a linear filter to `out_size`, bloomed with the world options' `bloom_intensity`, tone-mapped and written to `out_device` as sRGB
    /// RGBA8 (4 bytes a pixel) or, with `ffi::AIC_PRESENT_OUT_F16`, as four linear f16 (8 bytes a pixel). The info text is not drawn.
    ///
    /// # Safety
    /// `src_device` is a whole Split frame of the current viewport in device memory on the renderer's device, 8-byte aligned; `out_device` is device
    /// memory there of `out_size.width * out_size.height` elements, aligned to its element, not overlapping the frame.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub unsafe fn present_split(
        &mut self,
        src_device: *const core::ffi::c_void,
        out_device: *mut core::ffi::c_void,
        out_size: [u32; 2],
        flags: u32,
    ) -> Result<ffi::aic_present_info, RenderError> {
        let Device::One(ctx) = self.device else { panic!("present_split needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let options = options_of(self.cameras.cameras().world.options());
        let desc = ffi::aic_present_desc {
            src_width: viewport.framebuffer_size.width,
            src_height: viewport.framebuffer_size.height,
            out_width: out_size[0],
            out_height: out_size[1],
            bloom_intensity: options.bloom_intensity,
            tone_mapping: options.tone_mapping,
            maximum_intensity: options.maximum_intensity,
            flags,
        };
        let mut info = ffi::aic_present_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the target; the call returns when the image is written
        self.device.check(unsafe { ffi::aic_present_split(ctx.as_ptr(), &desc, src_device, out_device, 1, &mut info) })?;
        Ok(info)
    }

    /// The RGB-D export of the resident textures (`RerunImageExport::start_frame_copy`, all-is-cubes-gpu/src/rerun_image.rs:62-225,
    /// shaders/rerun-copy.wgsl): the resident Split frame at `src_device`, of the renderer's own viewport, resampled to `out_size` as sRGB RGBA8 into
    /// `color_device`, and its nearest depth texel unprojected to a distance along the view axis -- an `f32` per pixel, 0 where nothing was hit -- into
    /// `depth_device`. Either target may be null and is then not written. `out_size` `None`: `logged_image_size_policy` of the viewport
    /// (rerun_image.rs:302-311). Returns the size written and the report: how many pixels carry a surface, and their least and greatest distance. The
    /// pinhole and pose that go with the planes are `convert_camera_to_pinhole` of the world camera with its viewport set to the returned size.
    ///
    /// # Safety
    /// `src_device` is a whole Split frame of the current viewport in device memory on the renderer's device, 8-byte aligned; `color_device` and
    /// `depth_device` are null or device memory there of 4 bytes per output pixel, 4-byte aligned, overlapping neither the frame nor each other.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer.
    pub unsafe fn export_split(
        &mut self,
        src_device: *const core::ffi::c_void,
        color_device: *mut core::ffi::c_void,
        depth_device: *mut f32,
        out_size: Option<[u32; 2]>,
    ) -> Result<([u32; 2], ffi::aic_export_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("export_split needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        let ip = camera.projection_matrix().inverse().unwrap_or_default();
        let frame = viewport.framebuffer_size;
        let size = out_size.unwrap_or_else(|| {
            let mut logged = [frame.width, frame.height];
            // SAFETY: host arithmetic on two words; the cap is positive, so the call cannot fail
            let _ = unsafe { ffi::aic_export_size(frame.width, frame.height, 640.0 * 480.0, logged.as_mut_ptr()) };
            logged
        });
        let desc = ffi::aic_export_desc {
            src_width: frame.width,
            src_height: frame.height,
            out_width: size[0],
            out_height: size[1],
            inverse_projection_zw: [ip.m33 as f32, ip.m43 as f32, ip.m34 as f32, ip.m44 as f32],
            flags: 0,
            reserved: [0; 3],
        };
        let mut info = ffi::aic_export_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the targets; the call returns when the planes are written
        self.device.check(unsafe { ffi::aic_export_split(ctx.as_ptr(), &desc, src_device, color_device, depth_device, 1, &mut info) })?;
        Ok((size, info))
    }

    /// [`Self::present_split`] with the lines pass of `EverythingRenderer::draw_frame_linear` (all-is-cubes-gpu/src/everything.rs:616-658): `lines`,
    /// pairs of world-space vertices with a linear RGBA colour -- the cursor's wireframe from [`cursor_wireframe`], debug lines --, are drawn into the
    /// scene before bloom and tone mapping, depth-tested against the resident frame's depth plane, under the world camera's projection x view.
    /// Returns the presentation's report and how many lines, fragments and pixels were drawn.
    ///
    /// # Safety
    /// As [`Self::present_split`].
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer, or with more than `ffi::AIC_LINES_MAX` lines.
    pub unsafe fn present_split_lines(
        &mut self,
        src_device: *const core::ffi::c_void,
        out_device: *mut core::ffi::c_void,
        out_size: [u32; 2],
        flags: u32,
        lines: &[[ffi::aic_line_vertex; 2]],
    ) -> Result<(ffi::aic_present_info, ffi::aic_lines_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("present_split_lines needs a single-device renderer") };
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        let options = options_of(camera.options());
        let desc = ffi::aic_present_desc {
            src_width: viewport.framebuffer_size.width,
            src_height: viewport.framebuffer_size.height,
            out_width: out_size[0],
            out_height: out_size[1],
            bloom_intensity: options.bloom_intensity,
            tone_mapping: options.tone_mapping,
            maximum_intensity: options.maximum_intensity,
            flags,
        };
        // (euclid's row-vector order is WGSL's column-major one: all-is-cubes-gpu/src/camera.rs convert_matrix)
        let view_projection = camera.view_matrix().then(&camera.projection_matrix()).to_array().map(|v| v as f32);
        let lines_desc = ffi::aic_lines_desc {
            view_projection,
            n_lines: u32::try_from(lines.len()).expect("too many lines"),
            flags: 0,
            vertices: lines.as_ptr().cast(),
        };
        let mut info = ffi::aic_present_info::default();
        let mut lines_info = ffi::aic_lines_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the target; `lines` is copied before the call returns, and the call
        // returns when the image is written
        self.device.check(unsafe { ffi::aic_present_split_lines(ctx.as_ptr(), &desc, &lines_desc, src_device, out_device, 1, &mut info, &mut lines_info) })?;
        Ok((info, lines_info))
    }

    /// [`Self::present_split_lines`] with the info text of the interactive renderer laid over the tone-mapped scene on the device, as
    /// `postprocess_fragment` does (all-is-cubes-gpu/src/shaders/postprocess.wgsl:160-276): the font atlas is [`font_atlas`], set on the first call;
    /// the character grid is `character_texture_size` of the viewport's nominal size (text.rs:20-52) with the text's origin at (5, 5) nominal
    /// pixels (postprocess.rs:316-331), filled as `render_text_to_character_texture` fills it (text.rs:56-73); the text is empty when the options'
    /// `debug_info_text` is false (everything.rs:786-788). `lines`: `None` for no lines pass.
    ///
    /// # Safety
    /// As [`Self::present_split`].
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    ///
    /// # Panics
    /// On a multi-device renderer, with more than `ffi::AIC_LINES_MAX` lines, or with a viewport whose nominal size gives no character grid.
    pub unsafe fn present_split_text(
        &mut self,
        src_device: *const core::ffi::c_void,
        out_device: *mut core::ffi::c_void,
        out_size: [u32; 2],
        flags: u32,
        lines: Option<&[[ffi::aic_line_vertex; 2]]>,
        info_text: &str,
    ) -> Result<(ffi::aic_present_info, ffi::aic_lines_info), RenderError> {
        let Device::One(ctx) = self.device else { panic!("present_split_text needs a single-device renderer") };
        let cell = FONT_CELL;
        if !self.text_font_set {
            let (atlas, made_cell) = font_atlas();
            assert_eq!(made_cell, cell, "FontSystem16's character cell is 7 x 16");
            // SAFETY: the context is live; the atlas holds 16 x 16 cells of the size given and is copied before the call returns
            self.device.check(unsafe { ffi::aic_set_text_font(ctx.as_ptr(), atlas.as_ptr().cast(), cell[0], cell[1], cell[2]) })?;
            self.text_font_set = true;
        }
        let (viewport, _) = self.frame_desc();
        let camera = &self.cameras.cameras().world;
        let options = options_of(camera.options());
        let desc = ffi::aic_present_desc {
            src_width: viewport.framebuffer_size.width,
            src_height: viewport.framebuffer_size.height,
            out_width: out_size[0],
            out_height: out_size[1],
            bloom_intensity: options.bloom_intensity,
            tone_mapping: options.tone_mapping,
            maximum_intensity: options.maximum_intensity,
            flags,
        };
        let view_projection = camera.view_matrix().then(&camera.projection_matrix()).to_array().map(|v| v as f32);
        let lines_desc = lines.map(|lines| ffi::aic_lines_desc {
            view_projection,
            n_lines: u32::try_from(lines.len()).expect("too many lines"),
            flags: 0,
            vertices: lines.as_ptr().cast(),
        });
        let mut text_desc = ffi::aic_text_desc { scale: [0.0; 2], origin: [0.0; 2], cols: 0, rows: 0, flags: 0, codes: core::ptr::null() };
        let origin_px = [5.0f64, 5.0];
        // SAFETY: every pointer is to a local of the size the call writes
        let rc = unsafe {
            ffi::aic_text_geometry(
                viewport.nominal_size.width.into_inner(),
                viewport.nominal_size.height.into_inner(),
                cell[0],
                cell[1],
                cell[2],
                origin_px.as_ptr(),
                &mut text_desc.cols,
                &mut text_desc.rows,
                text_desc.scale.as_mut_ptr(),
                text_desc.origin.as_mut_ptr(),
            )
        };
        assert_eq!(rc, 0, "the viewport's nominal size gives no character grid");
        let shown = if camera.options().debug_info_text { info_text } else { "" };
        let mut codes = vec![0u8; text_desc.cols as usize * text_desc.rows as usize];
        // SAFETY: `codes` holds rows x cols bytes, which is what the call writes
        let rc = unsafe { ffi::aic_text_layout(shown.as_ptr().cast(), shown.len() as u64, text_desc.cols, text_desc.rows, codes.as_mut_ptr(), core::ptr::null_mut()) };
        assert_eq!(rc, 0, "aic_text_layout");
        text_desc.codes = codes.as_ptr();
        let mut info = ffi::aic_present_info::default();
        let mut lines_info = ffi::aic_lines_info::default();
        // SAFETY: the context is live; the caller vouches for the frame and the target; `lines` and `codes` are copied before the call returns, and
        // the call returns when the image is written
        self.device.check(unsafe {
            ffi::aic_present_split_text(
                ctx.as_ptr(),
                &desc,
                lines_desc.as_ref().map_or(core::ptr::null(), core::ptr::from_ref),
                &text_desc,
                src_device,
                out_device,
                1,
                &mut info,
                &mut lines_info,
            )
        })?;
        Ok((info, lines_info))
    }

    fn light_params(maximum_distance: u8, fast: bool, epsilon: u8, n_queue: i32, max_updates: u64) -> ffi::aic_light_params {
        ffi::aic_light_params {
            maximum_distance: i32::from(maximum_distance),
            fast: i32::from(fast),
            epsilon: i32::from(epsilon),
            batch: 32, // update_light_from_queue's batch with feature "auto-threads" (updater.rs:212-252)
            queue_order: QUEUE_ORDER,
            n_queue,
            lanes_per_cube: 0,
            hooks: 0,
            queue_cubes: core::ptr::null(),
            queue_priorities: core::ptr::null(),
            max_updates,
        }
    }

    /// Runs the light updater ON THE DEVICE against the world space as last uploaded: `Mutation::fast_evaluate_light`
    /// (if `fast`) and `Mutation::evaluate_light(epsilon, ..)` (space.rs:1496-1540) with
    /// `LightPhysics::Rays { maximum_distance }`. The device's light volume -- what the following frames trace -- is
    /// updated in place; the host `Space`'s light is not touched. Batches of 32 in the table order of the reference's
    /// queue, i.e. the texels `Space::evaluate_light` itself would produce with feature "auto-threads".
    /// Returns the number of cube updates.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    pub fn evaluate_light(&mut self, maximum_distance: u8, fast: bool, epsilon: u8) -> Result<u64, RenderError> {
        // n_queue = -1: without `fast`, start from every cube whose texel is Uninitialized (Priority::UNINIT)
        let params = Self::light_params(maximum_distance, fast, epsilon, -1, 0);
        let mut info = ffi::aic_light_info::default();
        self.device.evaluate_light(ffi::AIC_LAYER_WORLD, &params, &mut info)?;
        Ok(info.updates)
    }

    /// With [`Self::set_device_light`] on: continues the device's own update queue (what `update` queued for the blocks
    /// that changed, and what earlier calls left) for at most `max_updates` cube updates -- the per-frame slice of
    /// `Space::step`'s light update (updater.rs:181-290), on the device. Returns (updates done, queue entries left).
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    pub fn evaluate_light_budgeted(&mut self, max_updates: u64) -> Result<(u64, u32), RenderError> {
        let maximum_distance = self.device_light.expect("evaluate_light_budgeted needs set_device_light(Some(..))");
        // n_queue = 0: nothing new from the caller; the layer's queue is continued
        let params = Self::light_params(maximum_distance, false, 1, 0, max_updates);
        let mut info = ffi::aic_light_info::default();
        self.device.evaluate_light(ffi::AIC_LAYER_WORLD, &params, &mut info)?;
        Ok((info.updates, info.queue_left))
    }
}

impl HipRtRenderer {
    /// [`Self::evaluate_light_budgeted`] without blocking: the update runs on the library's worker thread beside the frames drawn
    /// meanwhile (which see the light as it stood); [`Self::finish_light_update`] -- or the next `update` -- publishes it. On a
    /// multi-device renderer the blocking call is made instead.
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    pub fn start_light_update(&mut self, max_updates: u64) -> Result<(), RenderError> {
        let maximum_distance = self.device_light.expect("start_light_update needs set_device_light(Some(..))");
        let params = Self::light_params(maximum_distance, false, 1, 0, max_updates);
        if !self.device.evaluate_light_submit(ffi::AIC_LAYER_WORLD, &params)? {
            let mut info = ffi::aic_light_info::default();
            self.device.evaluate_light(ffi::AIC_LAYER_WORLD, &params, &mut info)?;
        }
        Ok(())
    }

    /// Waits for the update [`Self::start_light_update`] began and makes its light current. Returns (updates done, queue entries left).
    ///
    /// # Errors
    /// As [`HeadlessRenderer::draw`] for device failures.
    pub fn finish_light_update(&mut self) -> Result<(u64, u32), RenderError> {
        let mut info = ffi::aic_light_info::default();
        self.device.evaluate_light_wait(ffi::AIC_LAYER_WORLD, &mut info)?;
        Ok((info.updates, info.queue_left))
    }
}

/// `PixelPicker` of raytrace_to_texture.rs:838-908: the order in which the incremental renderer takes a frame's pixels -- centre first and dithered
/// (`aic_pixel_order`), the central pixels interleaved with the rest. An iterator over pixel indices `y * width + x` that never ends; after
/// `cycle_length()` picks every pixel has been picked. Feed `take(rays_per_frame)` of it to [`HipRtRenderer::trace_pixels`].
#[derive(Clone, Debug)]
pub struct PixelPicker {
    size: (u32, u32),
    order: Box<[u32]>,
    central: u64,
    cycle_length: u64,
    next: u64,
}

impl PixelPicker {
    /// # Panics
    /// If the viewport has more than `u32::MAX` pixels.
    pub fn new(width: u32, height: u32) -> Self {
        let mut order = vec![0u32; (width as usize) * (height as usize)].into_boxed_slice();
        let (mut central, mut cycle_length) = (0u32, 0u64);
        // SAFETY: `order` holds width * height entries (a null pointer asks for none); the other two are valid out-pointers
        let rc = unsafe {
            ffi::aic_pixel_order(width, height, if order.is_empty() { core::ptr::null_mut() } else { order.as_mut_ptr() }, &mut central, &mut cycle_length)
        };
        assert_eq!(rc, ffi::AIC_OK, "aic_pixel_order({width}, {height})");
        Self { size: (width, height), order, central: u64::from(central), cycle_length, next: 0 }
    }

    /// Starts over with the new size, if it differs (as the reference's `resize`).
    pub fn resize(&mut self, width: u32, height: u32) {
        if self.size != (width, height) {
            *self = Self::new(width, height);
        }
    }

    /// After at least this many picks, the entire image has been covered.
    pub fn cycle_length(&self) -> u64 {
        self.cycle_length
    }
}

impl Iterator for PixelPicker {
    type Item = u32;

    fn next(&mut self) -> Option<u32> {
        let count = self.order.len() as u64;
        if count == 0 {
            return None;
        }
        let (k, half) = (self.next, self.next / 2);
        self.next += 1;
        // itertools::Interleave of the two cycles; with no central pixels the inner side is empty and every pick is the outer's
        let index = if self.central == 0 {
            k % count
        } else if k % 2 == 0 {
            half % self.central
        } else {
            self.central + half % (count - self.central)
        };
        Some(self.order[index as usize])
    }
}

/// A frame in flight ([`HipRtRenderer::begin_frame`]): the host buffer the library fills, and what wrapping it needs. Dropping it without
/// `finish_frame` leaves the slot busy until the renderer is dropped (the library waits for it then).
pub struct PendingFrame {
    slot: u32,
    streamed: bool,
    viewport: Viewport,
    data: Vec<[u8; 4]>,
    info: ffi::aic_frame_info,
}

/// `draw_info_text` of the reference (raytracer/renderer.rs:659-683, private there): the info text over the finished frame,
/// `FontSystem16` glyphs at offset (5, 5), outline in `paint[0]`, glyph pixels in `paint[1]`.
fn draw_info_text(output: &mut [[u8; 4]], viewport: Viewport, paint: &[[u8; 4]; 2], info_text: &str) {
    let size = viewport.framebuffer_size;
    let font = universe::Builtin::FontSystem16.read::<text::FontDef>();
    font.draw_str_monospaced(info_text, |pixel, value| {
        let (x, y) = (pixel.x + 5, pixel.y + 5);
        if x >= 0 && y >= 0 && (x as u32) < size.width && (y as u32) < size.height {
            output[y as usize * size.width as usize + x as usize] = paint[match value {
                text::Value::Outline => 0,
                text::Value::Foreground => 1,
            }];
        }
    });
}

impl Drop for HipRtRenderer {
    fn drop(&mut self) {
        self.device.destroy();
    }
}

impl HeadlessRenderer for HipRtRenderer {
    fn update(&mut self, read_tickets: Layers<ReadTicket<'_>>, cursor: Option<&Cursor>) -> Result<(), RenderError> {
        self.update_scene(read_tickets, cursor)
    }

    fn draw<'a>(&'a mut self, info_text: &'a str) -> BoxFuture<'a, Result<Rendering, RenderError>> {
        // `draw` must not touch the universe (headless.rs:36-38): everything it needs was forwarded by `update`
        Box::pin(async move { self.draw_rgba(info_text) })
    }
}

/// `character::exposure::State` (all-is-cubes/src/character/exposure.rs:37-151) over the library's `aic_exposure_state`: what a host that steps no
/// `Character` keeps to drive `GraphicsOptions::exposure = Automatic`. Once per simulation step, `step`, then hand `exposure()` to
/// `Camera::set_measured_exposure`.
#[derive(Clone, Debug)]
pub struct ExposureState(ffi::aic_exposure_state);

impl Default for ExposureState {
    fn default() -> Self {
        let mut s = ffi::aic_exposure_state { luminance_samples: [1.0; 100], luminance_sample_index: 0, exposure_log: 0.0 };
        // SAFETY: a valid pointer to a state
        let _ = unsafe { ffi::aic_exposure_init(&mut s) };
        Self(s)
    }
}

impl ExposureState {
    /// `State::exposure`
    pub fn exposure(&self) -> f32 {
        let (mut copy, mut e) = (self.0, 1.0f32);
        // SAFETY: valid pointers; `dt == 0` only reads the state
        let _ = unsafe { ffi::aic_exposure_advance(&mut copy, 0, core::ptr::null(), 0.0, &mut e) };
        e
    }

    /// The ring of luminance samples.
    pub fn samples(&self) -> &[f32; 100] {
        &self.0.luminance_samples
    }

    /// `State::step`: samples the renderer's world space from `view_transform` and eases the exposure towards its target. `maximum_distance` is that of
    /// the space's `LightPhysics::Rays`, `None` for `LightPhysics::None`. `dt == 0` does nothing.
    ///
    /// # Errors
    /// As [`HipRtRenderer::sample_luminance`].
    pub fn step(&mut self, renderer: &mut HipRtRenderer, view_transform: ViewTransform, maximum_distance: Option<u8>, dt: f64) -> Result<(), RenderError> {
        if dt == 0. {
            return Ok(());
        }
        let max_steps = maximum_distance.map_or(0, |d| u32::from(d) * 2);
        let r = view_transform.rotation;
        let t = view_transform.translation;
        let mut rays = [[0.0f64; 6]; ffi::AIC_EXPOSURE_RAYS as usize];
        let first = (self.0.luminance_sample_index + 1) % ffi::AIC_EXPOSURE_SAMPLES;
        // SAFETY: four and three doubles in, AIC_EXPOSURE_RAYS x 6 doubles out
        let rc = unsafe { ffi::aic_exposure_rays([r.i, r.j, r.k, r.r].as_ptr(), [t.x, t.y, t.z].as_ptr(), first, ffi::AIC_EXPOSURE_RAYS, rays.as_mut_ptr().cast()) };
        assert_eq!(rc, ffi::AIC_OK);
        let samples = renderer.sample_luminance(ffi::AIC_LAYER_WORLD, &rays, max_steps)?;
        // SAFETY: the samples hold AIC_EXPOSURE_RAYS floats
        let rc = unsafe { ffi::aic_exposure_advance(&mut self.0, ffi::AIC_EXPOSURE_RAYS, samples.as_ptr(), dt, core::ptr::null_mut()) };
        assert_eq!(rc, ffi::AIC_OK);
        Ok(())
    }
}

/// A mutex-wrapped renderer for call sites that need `Sync` (e.g. the recording thread, record.rs:97-113).
pub type SharedHipRtRenderer = Arc<Mutex<HipRtRenderer>>;
