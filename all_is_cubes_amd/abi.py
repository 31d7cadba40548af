"""ctypes binding of the C ABI in include/aic_hip.h (libaic_hip.so).

This is plumbing for the Python-side tests and bench: it adds nothing to the boundary.
There is NO fallback: if the HIP library is missing or no MI355X is usable the calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
from pathlib import Path
from typing import Optional

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libaic_hip.so"

AIC_OK = 0
ERR_NAMES = {1: "AIC_ERR_INVALID", 2: "AIC_ERR_NO_DEVICE", 3: "AIC_ERR_OOM", 4: "AIC_ERR_DEVICE", 5: "AIC_ERR_UNSUPPORTED"}
LAYER_WORLD, LAYER_UI = 0, 1
MAX_IN_FLIGHT = 32  # AIC_MAX_IN_FLIGHT
FLAW_UNSUPPORTED, FLAW_NO_BLOOM = 1, 2
FRAME_COUNTERS, FRAME_AUX, FRAME_PIXEL_CENTERS, FRAME_OUT_LINEAR, FRAME_OUT_COLORBUF, FRAME_NO_FEEDBACK = 1, 2, 4, 8, 16, 32
FRAME_BLOOM = 64  # AIC_FRAME_BLOOM: bloom the frame when the world options' bloom_intensity > 0 (RGBA8 output, whole frames)
FRAME_OUT_SPLIT = 512  # AIC_FRAME_OUT_SPLIT: an f16x4 colour plane and an f32 depth plane (12 bytes per pixel), raytrace_to_texture's two texels
RAYS_NO_SKY, RAYS_DEVICE = 128, 256  # aic_trace_rays only: include_sky = false; rays / out / aux are device pointers
MAX_RAYS = 2048 * 65535  # rays in one aic_trace_rays call
PIXELS_DEVICE, PIXELS_IN_PLACE = 1, 2  # aic_trace_pixels' mode: pixels / out / aux are device pointers; out is a whole frame written at the listed pixels
MAX_PIXELS = 2048 * 65535  # pixels in one aic_trace_pixels call
REPROJECT_KEEP_SPLATS = 1  # AIC_REPROJECT_KEEP_SPLATS: reprojected texels stay at full resolution; only the gaps take the fill
REPROJECT_MAX_LEVELS = 12  # AIC_REPROJECT_MAX_LEVELS
PRESENT_OUT_F16 = 1  # AIC_PRESENT_OUT_F16: the presented image as four f16 per pixel, linear, alpha 1.0, instead of sRGB RGBA8
PRESENT_MAX_PIXELS = 1 << 31  # AIC_PRESENT_MAX_PIXELS
STALE_DEPTH_TEST = 1  # AIC_STALE_DEPTH_TEST: a rectangle keeps out an opaque world pixel whose depth lies in front of it
STALE_MAX_RECTS = 4096  # AIC_STALE_MAX_RECTS
STALE_DEPTH_BEHIND = 2  # AIC_STALE_DEPTH_BEHIND (aic_pick_stale_cubes): a light cube's rectangle keeps out a world pixel whose nearest surface lies behind it
LINES_DEVICE = 1  # AIC_LINES_DEVICE: the line vertices are a device pointer
LINES_MAX = 1 << 20  # AIC_LINES_MAX
CURSOR_MAX_LINES = 28  # AIC_CURSOR_MAX_LINES
TEXT_DEVICE = 1  # AIC_TEXT_DEVICE: the character codes are a device pointer
# terminal frames (aic_image_cells, aic_render_cells, aic_cells_ansi): CharacterMode, ColorMode, the flags and a cell's colour kinds
CELLS_NAMES, CELLS_SHADES, CELLS_SPLIT, CELLS_SHAPES, CELLS_BRAILLE = 0, 1, 2, 3, 4
CELLS_COLOR_NONE, CELLS_COLOR_256, CELLS_COLOR_RGB = 0, 1, 2
CELLS_IMAGE_DEVICE, CELLS_OUT_DEVICE, CELLS_IMAGE_F16, CELLS_POSTPROCESSED = 1, 2, 4, 8
CELLS_ANSI_IN_RECT = 1
CELL_GLYPH_BLOCK = 0x80000000  # AIC_CELL_GLYPH_BLOCK | layer << 16 | block_index: the text of that block of that layer
CELL_COLOR_NONE, CELL_COLOR_RESET, CELL_COLOR_BLACK, CELL_COLOR_ANSI, CELL_COLOR_RGB = 0, 1, 2, 3, 4
# aic_frame_desc.tuning / aic_frame_info.variant (include/aic_hip.h)
TUNE_QUEUES_SHIFT, TUNE_SUPER_SHIFT, TUNE_VARIANT_SHIFT = 0, 4, 9
VARIANT_AUTO, VARIANT_PLAIN, VARIANT_EXCHANGING, VARIANT_RECORDING = 0, 1, 2, 3
LIGHT_HOOK_SESSION, LIGHT_HOOK_POOL_SHIFT = 1, 8


def bloom_geometry(width: int, height: int):
    """(levels, (T0x, T0y)) of AIC_FRAME_BLOOM's mip chain for a width x height frame (mip_ping.rs:460-481 on the half-size request of
    bloom.rs:50-53): R = (ceil(w / 2), ceil(h / 2)), L = min(6, ilog2(min R) + 1), T0 = R rounded up to a multiple of 2^L."""
    rx, ry = (width + 1) // 2, (height + 1) // 2
    levels = min(6, min(rx, ry).bit_length())
    d = 1 << levels
    return levels, ((rx + d - 1) // d * d, (ry + d - 1) // d * d)


def split_planes(buf, rows: int, width: int):
    """The two planes of an AIC_FRAME_OUT_SPLIT buffer of rows x width pixels (12 bytes each; `buf`: anything numpy can view as bytes, e.g. what a
    submitted frame left in device memory, copied to the host): {"color_f16": [rows, width, 4] float16, "depth": [rows, width] float32}."""
    raw = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    n = int(rows) * int(width)
    if raw.size < n * 12:
        raise ValueError(f"a Split frame of {rows} x {width} pixels is {n * 12} bytes, the buffer has {raw.size}")
    return {"color_f16": raw[:n * 8].view(np.float16).reshape(rows, width, 4), "depth": raw[n * 8:n * 12].view(np.float32).reshape(rows, width)}


def tuning(queues=None, super_shift=None, variant=None) -> int:
    """aic_frame_desc.tuning: the number of tile queues (1..8), the super-block edge in macro tiles (log2) and the production variant of the
    trace kernel (VARIANT_*); None leaves the library's choice. Any value gives the same image."""
    t = 0
    if queues is not None:
        t |= (int(queues) & 15) << TUNE_QUEUES_SHIFT
    if super_shift is not None:
        t |= ((int(super_shift) + 1) & 31) << TUNE_SUPER_SHIFT
    if variant is not None:
        t |= (int(variant) & 3) << TUNE_VARIANT_SHIFT
    return t

# every symbol include/aic_hip.h declares
ABI_SYMBOLS = [
    "aic_abi_version", "aic_create", "aic_destroy", "aic_last_error", "aic_device_name", "aic_upload_space",
    "aic_clear_space", "aic_update_cubes", "aic_update_light_volume", "aic_replace_block", "aic_replace_blocks", "aic_compact", "aic_set_options", "aic_set_depth_transform",
    "aic_render", "aic_render_submit", "aic_render_wait", "aic_render_submit_batch", "aic_render_wait_batch", "aic_trace_patches", "aic_trace_rays", "aic_trace_pixels", "aic_pixel_order", "aic_reproject_split", "aic_reproject_geometry", "aic_pick_pixels", "aic_stale_rects", "aic_pick_stale", "aic_pick_stale_cubes", "aic_probe_stale_cube_rects", "aic_find_block_cubes", "aic_pick_stale_blocks", "aic_replace_cube_grid", "aic_copy_cube_grid", "aic_update_light_volume_device", "aic_present_split", "aic_present_geometry", "aic_present_split_lines", "aic_present_lines_scratch", "aic_cursor_wireframe", "aic_cursor_raycast", "aic_light_rays", "aic_light_rays_bound", "aic_light_rays_wireframe", "aic_light_rays_cursor_lines", "aic_cells_geometry", "aic_image_cells", "aic_render_cells", "aic_cells_ansi", "aic_set_text_font", "aic_text_geometry", "aic_text_layout", "aic_present_split_text", "aic_export_split", "aic_export_size", "aic_exposure_init", "aic_exposure_rays", "aic_sample_luminance", "aic_exposure_advance", "aic_partition_rows", "aic_assemble_strips", "aic_assemble_strips_async", "aic_assemble_strips_on", "aic_read_aux", "aic_synchronize", "aic_stream", "aic_wait_event", "aic_stream_wait_frame",
    "aic_probe_raycast", "aic_probe_light_lut", "aic_probe_powf", "aic_probe_expf", "aic_probe_bloom",
    "aic_ortho_image_size", "aic_render_orthographic",
    "aic_evaluate_light", "aic_evaluate_light_submit", "aic_evaluate_light_wait", "aic_evaluate_light_poll", "aic_light_cubes_changed", "aic_light_changed_count", "aic_light_changed_take", "aic_read_light_volume", "aic_read_light_cubes", "aic_light_chart", "aic_probe_derived", "aic_probe_log2f", "aic_probe_cube_grid",
    "aic_create_multi", "aic_destroy_multi", "aic_multi_device_count", "aic_multi_context", "aic_multi_last_error", "aic_multi_upload_space",
    "aic_multi_clear_space", "aic_multi_update_cubes", "aic_multi_update_light_volume", "aic_multi_evaluate_light", "aic_multi_light_cubes_changed", "aic_multi_replace_blocks", "aic_multi_set_options", "aic_multi_set_depth_transform",
    "aic_multi_render", "aic_multi_render_submit", "aic_multi_render_wait",
]


class AicError(RuntimeError):
    """Maps to `RenderError` on the reference side (all-is-cubes-render/src/lib.rs:46-54)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {message}")
        self.code = code


class BlockDesc(C.Structure):
    _fields_ = [("resolution", C.c_int32), ("vlo", C.c_int32 * 3), ("vsize", C.c_int32 * 3), ("vox_off", C.c_uint32),
                ("pal_off", C.c_uint32), ("pal_len", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_int32)]


class LightParams(C.Structure):
    _fields_ = [("maximum_distance", C.c_int32), ("fast", C.c_int32), ("epsilon", C.c_int32), ("batch", C.c_int32),
                ("queue_order", C.c_int32), ("n_queue", C.c_int32), ("lanes_per_cube", C.c_int32), ("hooks", C.c_int32), ("queue_cubes", C.c_void_p), ("queue_priorities", C.c_void_p),
                ("max_updates", C.c_uint64)]


class LightInfo(C.Structure):
    _fields_ = [("updates", C.c_uint64), ("batches", C.c_uint64), ("cost", C.c_uint64), ("device_ms", C.c_double),
                ("total_ms", C.c_double), ("queue_left", C.c_uint32), ("pad", C.c_uint32), ("bundles_visited", C.c_uint64)]


def light_chart():
    """The light propagation chart the library generates (chart/generator.rs): (weights [n,6] f32, children [n,6] u32, depth).
    Host-only: needs no device."""
    lib = load()
    lib.aic_light_chart.restype = C.c_uint32
    lib.aic_light_chart.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    depth = C.c_uint32(0)
    n = lib.aic_light_chart(None, None, C.byref(depth))
    w = np.zeros((n, 6), np.float32)
    ch = np.zeros((n, 6), np.uint32)
    lib.aic_light_chart(w.ctypes.data, ch.ctypes.data, C.byref(depth))
    return w, ch, int(depth.value)


def pixel_order(width: int, height: int):
    """PixelPicker::new (raytrace_to_texture.rs:856-891) through aic_pixel_order: (order [width * height] uint32 -- the pixel indices y * width + x, centre
    first and dithered --, central, cycle_length). Pick k of the sequence is order[(k // 2) % central] for even k and
    order[central + (k // 2) % (count - central)] for odd k; with central = 0, order[k % count]. Host-only: needs no device or context."""
    lib = load()
    lib.aic_pixel_order.restype = C.c_int
    lib.aic_pixel_order.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    order = np.zeros(int(width) * int(height), np.uint32)
    central, cycle = C.c_uint32(0), C.c_uint64(0)
    rc = lib.aic_pixel_order(int(width), int(height), order.ctypes.data if order.size else None, C.byref(central), C.byref(cycle))
    if rc != 0:
        raise AicError(rc, f"aic_pixel_order({width}, {height})")
    return order, int(central.value), int(cycle.value)


def stale_rects(view_projection, width: int, height: int, boxes, expand: int = 1) -> np.ndarray:
    """Boxes of changed cubes as the screen rectangles of the pixels they can have changed (aic_stale_rects): [n] STALE_RECT_DTYPE records for
    pick_stale. `view_projection`: camera.projection * camera.view_matrix, column-major, 16 doubles; `boxes`: [n, 6] int32 (lower, upper exclusive cube
    bounds); `expand`: cubes the box is grown by on every side -- 1 covers the light stencil and ambient occlusion at a surface beside a changed cube.
    Host-only: needs no device or context."""
    lib = load()
    lib.aic_stale_rects.restype = C.c_int
    lib.aic_stale_rects.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]
    m = (C.c_double * 16)(*[float(v) for v in np.asarray(view_projection, np.float64).reshape(16)])
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 6))
    out = np.zeros(len(b), STALE_RECT_DTYPE)
    rc = lib.aic_stale_rects(m, int(width), int(height), len(b), b.ctypes.data if len(b) else None, int(expand), out.ctypes.data if len(b) else None)
    if rc != 0:
        raise AicError(rc, "aic_stale_rects")
    return out


def reproject_geometry(width: int, height: int):
    """The gap-fill chain of aic_reproject_split for a width x height frame (aic_reproject_geometry): (levels L, (T0x, T0y), bytes of context scratch the
    call allocates). Host-only: needs no device or context."""
    lib = load()
    lib.aic_reproject_geometry.restype = C.c_int
    lib.aic_reproject_geometry.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    levels, t0, scratch = C.c_uint32(0), (C.c_uint32 * 2)(0, 0), C.c_uint64(0)
    rc = lib.aic_reproject_geometry(int(width), int(height), C.byref(levels), t0, C.byref(scratch))
    if rc != 0:
        raise AicError(rc, f"aic_reproject_geometry({width}, {height})")
    return int(levels.value), (int(t0[0]), int(t0[1])), int(scratch.value)


def present_geometry(src_size, out_size):
    """The bloom chain of aic_present_split for a (width, height) Split frame shown in an (width, height) window (aic_present_geometry): (levels L,
    (T0x, T0y), bytes of context scratch a call with bloom_intensity > 0 allocates; a call with 0 allocates none). Host-only: needs no device or context."""
    lib = load()
    lib.aic_present_geometry.restype = C.c_int
    lib.aic_present_geometry.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    levels, t0, scratch = C.c_uint32(0), (C.c_uint32 * 2)(0, 0), C.c_uint64(0)
    rc = lib.aic_present_geometry(int(src_size[0]), int(src_size[1]), int(out_size[0]), int(out_size[1]), C.byref(levels), t0, C.byref(scratch))
    if rc != 0:
        raise AicError(rc, f"aic_present_geometry({tuple(src_size)}, {tuple(out_size)})")
    return int(levels.value), (int(t0[0]), int(t0[1])), int(scratch.value)


def present_lines_scratch(src_size, out_size, n_lines: int) -> int:
    """Bytes of line scratch an aic_present_split_lines call with `n_lines` host vertices pairs allocates on top of present_geometry's figure
    (aic_present_lines_scratch). Host-only: needs no device or context."""
    lib = load()
    lib.aic_present_lines_scratch.restype = C.c_int
    lib.aic_present_lines_scratch.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint64)]
    scratch = C.c_uint64(0)
    rc = lib.aic_present_lines_scratch(int(src_size[0]), int(src_size[1]), int(out_size[0]), int(out_size[1]), int(n_lines), C.byref(scratch))
    if rc != 0:
        raise AicError(rc, f"aic_present_lines_scratch({tuple(src_size)}, {tuple(out_size)}, {n_lines})")
    return int(scratch.value)


def export_size(size, max_area: float = 640.0 * 480.0):
    """The size an exported image of a `size` = (width, height) frame is logged at (aic_export_size; logged_image_size_policy, rerun_image.rs:302-311): the
    size itself when its area is at most `max_area`, else scaled by sqrt(max_area / area) and rounded up per axis. Host-only: needs no device or context."""
    lib = load()
    out = (C.c_uint32 * 2)(0, 0)
    rc = lib.aic_export_size(int(size[0]), int(size[1]), float(max_area), out)
    if rc != 0:
        raise AicError(rc, f"aic_export_size({tuple(size)}, {max_area})")
    return int(out[0]), int(out[1])


class SpaceDesc(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("size", C.c_int32 * 3), ("block_index", C.c_void_p), ("light", C.c_void_p),
                ("n_blocks", C.c_uint32), ("blocks", C.c_void_p), ("voxels", C.c_void_p), ("n_voxels", C.c_uint64),
                ("palette", C.c_void_p), ("n_palette", C.c_uint64), ("sky_kind", C.c_int32), ("sky", (C.c_float * 3) * 8),
                ("block_sky", (C.c_uint8 * 4) * 7)]


class Options(C.Structure):
    _fields_ = [("fog", C.c_int32), ("transparency", C.c_int32), ("threshold", C.c_float), ("lighting", C.c_int32),
                ("bounce_samples", C.c_int32), ("antialiasing", C.c_int32), ("debug_pixel_cost", C.c_int32),
                ("tone_mapping", C.c_int32), ("maximum_intensity", C.c_float), ("bloom_intensity", C.c_float),
                ("view_distance", C.c_double)]


class Camera(C.Structure):
    _fields_ = [("inverse_projection_view", C.c_double * 16), ("exposure", C.c_float), ("reserved", C.c_int32)]


class Partition(C.Structure):
    _fields_ = [("strip_rows", C.c_uint32), ("n_parts", C.c_uint32), ("part", C.c_uint32), ("reserved", C.c_uint32)]


class FrameDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("world", Camera), ("ui", Camera), ("backdrop", C.c_float * 4),
                ("partition", Partition), ("flags", C.c_uint32), ("tuning", C.c_uint32)]


class FrameInfo(C.Structure):
    _fields_ = [("cubes_traced", C.c_uint64), ("n_outer", C.c_uint64), ("n_inner", C.c_uint64), ("n_hits", C.c_uint64),
                ("n_light", C.c_uint64), ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("rows_rendered", C.c_uint32),
                ("flaws", C.c_uint32), ("variant", C.c_uint32), ("tile_queues", C.c_uint32)]


class ReprojectDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("reprojection", C.c_float * 16), ("inverse_projection_zw", C.c_float * 4),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ReprojectInfo(C.Structure):
    _fields_ = [("n_splats", C.c_uint64), ("n_dropped", C.c_uint64), ("n_gaps", C.c_uint64), ("n_unfilled", C.c_uint64),
                ("kernel_ms", C.c_float), ("levels", C.c_uint32), ("t0", C.c_uint32 * 2)]


class PickDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n", C.c_uint32), ("max_unknown", C.c_uint32), ("skip_unknown", C.c_uint64),
                ("cursor", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PickInfo(C.Structure):
    _fields_ = [("n_unknown", C.c_uint64), ("next_cursor", C.c_uint64), ("n_from_unknown", C.c_uint32), ("n_from_order", C.c_uint32),
                ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


class StaleRect(C.Structure):
    _fields_ = [("x0", C.c_uint16), ("y0", C.c_uint16), ("x1", C.c_uint16), ("y1", C.c_uint16), ("dmin", C.c_float), ("reserved", C.c_uint32)]


STALE_RECT_DTYPE = np.dtype([("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2"), ("dmin", "<f4"), ("reserved", "<u4")])


class StaleDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n", C.c_uint32), ("max_stale", C.c_uint32), ("skip_stale", C.c_uint64),
                ("cursor", C.c_uint64), ("n_rects", C.c_uint32), ("flags", C.c_uint32), ("rects", C.c_void_p)]


class StaleInfo(C.Structure):
    _fields_ = [("n_stale", C.c_uint64), ("next_cursor", C.c_uint64), ("n_from_stale", C.c_uint32), ("n_from_order", C.c_uint32),
                ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


class StaleCubesDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n", C.c_uint32), ("max_stale", C.c_uint32), ("skip_stale", C.c_uint64),
                ("cursor", C.c_uint64), ("view_projection", C.c_double * 16), ("n_boxes", C.c_uint32), ("expand", C.c_int32),
                ("n_light_cubes", C.c_uint32), ("flags", C.c_uint32), ("boxes", C.c_void_p), ("light_cubes", C.c_void_p)]


class StaleCubesInfo(C.Structure):
    _fields_ = [("n_stale", C.c_uint64), ("next_cursor", C.c_uint64), ("n_from_stale", C.c_uint32), ("n_from_order", C.c_uint32),
                ("kernel_ms", C.c_float), ("reserved", C.c_uint32), ("n_rects", C.c_uint32), ("whole_frame", C.c_uint32)]


class BlockCubesInfo(C.Structure):
    _fields_ = [("n_cubes", C.c_uint64), ("n_runs", C.c_uint64), ("bounds", C.c_int32 * 6), ("n_written", C.c_uint32), ("merged", C.c_uint32),
                ("kernel_ms", C.c_float), ("reserved", C.c_uint32)]


class StaleBlocksDesc(C.Structure):
    _fields_ = [("cubes", StaleCubesDesc), ("layer", C.c_int32), ("n_blocks", C.c_uint32), ("block_indices", C.c_void_p), ("max_runs", C.c_uint32),
                ("reserved", C.c_uint32)]


class StaleBlocksInfo(C.Structure):
    _fields_ = [("pick", StaleCubesInfo), ("found", BlockCubesInfo)]


STALE_CUBE_RECT_DTYPE = np.dtype([("x0", "<u4"), ("y0", "<u4"), ("x1", "<u4"), ("y1", "<u4"), ("dmin", "<f4"), ("dmax", "<f4")])


class PresentDesc(C.Structure):
    _fields_ = [("src_width", C.c_uint32), ("src_height", C.c_uint32), ("out_width", C.c_uint32), ("out_height", C.c_uint32),
                ("bloom_intensity", C.c_float), ("tone_mapping", C.c_int32), ("maximum_intensity", C.c_float), ("flags", C.c_uint32)]


class PresentInfo(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("levels", C.c_uint32), ("t0", C.c_uint32 * 2), ("bloomed", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class ExportDesc(C.Structure):
    _fields_ = [("src_width", C.c_uint32), ("src_height", C.c_uint32), ("out_width", C.c_uint32), ("out_height", C.c_uint32),
                ("inverse_projection_zw", C.c_float * 4), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class ExportInfo(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("n_surface", C.c_uint32), ("depth_min", C.c_float), ("depth_max", C.c_float), ("reserved", C.c_uint32 * 4)]


class LinesDesc(C.Structure):
    _fields_ = [("view_projection", C.c_float * 16), ("n_lines", C.c_uint32), ("flags", C.c_uint32), ("vertices", C.c_void_p)]


class LinesInfo(C.Structure):
    _fields_ = [("n_clipped_away", C.c_uint64), ("n_fragments", C.c_uint64), ("n_passed", C.c_uint64), ("n_pixels", C.c_uint64)]


class TextDesc(C.Structure):
    _fields_ = [("scale", C.c_float * 2), ("origin", C.c_float * 2), ("cols", C.c_uint32), ("rows", C.c_uint32), ("flags", C.c_uint32), ("codes", C.c_void_p)]


EXPOSURE_SAMPLES, EXPOSURE_RAYS = 100, 10  # State::luminance_samples; rays per step (exposure.rs)


class ExposureStateC(C.Structure):  # aic_exposure_state
    _fields_ = [("luminance_samples", C.c_float * 100), ("luminance_sample_index", C.c_uint32), ("exposure_log", C.c_float)]


def exposure_rays(rotation_ijkr, translation, first_index: int, n: int = EXPOSURE_RAYS) -> np.ndarray:
    """The rays of one step of character::exposure::State::step (aic_exposure_rays; exposure.rs:85-105): [n,6] f64 = (origin xyz, direction xyz), ray k
    for sample index (first_index + k) % 100, under the view transform (rotation quaternion i, j, k, r; translation). Host-only."""
    lib = load()
    lib.aic_exposure_rays.restype = C.c_int
    lib.aic_exposure_rays.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.c_uint32, C.c_void_p]
    q = (C.c_double * 4)(*[float(v) for v in rotation_ijkr])
    t = (C.c_double * 3)(*[float(v) for v in translation])
    rays = np.zeros((int(n), 6), np.float64)
    rc = lib.aic_exposure_rays(q, t, int(first_index), int(n), rays.ctypes.data if rays.size else None)
    if rc != 0:
        raise AicError(rc, "aic_exposure_rays")
    return rays


class ExposureState:
    """character::exposure::State (exposure.rs:37-151) over aic_exposure_state: the ring of 100 luminance samples, the index last written and the log of
    the exposure. `advance` takes the samples of one step (Context.sample_luminance of `rays()`); everything here is host-only."""

    def __init__(self):
        self.c = ExposureStateC()
        lib = load()
        lib.aic_exposure_init.restype = C.c_int
        lib.aic_exposure_init.argtypes = [C.POINTER(ExposureStateC)]
        lib.aic_exposure_advance.restype = C.c_int
        lib.aic_exposure_advance.argtypes = [C.POINTER(ExposureStateC), C.c_uint32, C.c_void_p, C.c_double, C.POINTER(C.c_float)]
        rc = lib.aic_exposure_init(C.byref(self.c))
        if rc != 0:
            raise AicError(rc, "aic_exposure_init")

    @property
    def samples(self) -> np.ndarray:
        return np.array(self.c.luminance_samples[:], np.float32)

    @property
    def index(self) -> int:
        return int(self.c.luminance_sample_index)

    @property
    def exposure_log(self) -> np.float32:
        return np.float32(self.c.exposure_log)

    def rays(self, rotation_ijkr, translation, n: int = EXPOSURE_RAYS) -> np.ndarray:
        """The next `n` rays of the ring: those of the sample indices the next advance() writes."""
        return exposure_rays(rotation_ijkr, translation, (self.index + 1) % EXPOSURE_SAMPLES, n)

    def advance(self, samples, dt: float) -> np.float32:
        """Stores the samples, eases the exposure towards its target by `dt` seconds (dt == 0: nothing) and returns the exposure (aic_exposure_advance)."""
        smp = np.ascontiguousarray(samples, np.float32).reshape(-1)
        out = C.c_float(0)
        rc = load().aic_exposure_advance(C.byref(self.c), len(smp), smp.ctypes.data if smp.size else None, float(dt), C.byref(out))
        if rc != 0:
            raise AicError(rc, "aic_exposure_advance")
        return np.float32(out.value)

    def exposure(self) -> np.float32:
        return self.advance([], 0.0)


class CursorDesc(C.Structure):
    _fields_ = [("cube", C.c_int32 * 3), ("face_entered", C.c_int32), ("face_selected", C.c_int32), ("point_entered", C.c_double * 3),
                ("distance_to_point", C.c_double), ("voxel_lo", C.c_int32 * 3), ("voxel_size", C.c_int32 * 3), ("resolution", C.c_int32),
                ("reserved", C.c_int32)]


# aic_cursor_hit: 144 bytes, the first 88 an aic_cursor_desc (CursorDesc)
CURSOR_HIT_DTYPE = np.dtype({
    "names": ["cube", "face_entered", "face_selected", "point_entered", "distance_to_point", "voxel_lo", "voxel_size", "resolution", "reserved", "hit",
              "block_index", "voxel", "has_preceding", "preceding_cube", "preceding_block_index", "light_hit", "light_preceding", "steps", "reserved_hit"],
    "formats": [("<i4", (3,)), "<i4", "<i4", ("<f8", (3,)), "<f8", ("<i4", (3,)), ("<i4", (3,)), "<i4", "<i4", "<i4",
                "<u4", ("<i4", (3,)), "<i4", ("<i4", (3,)), "<u4", ("u1", (4,)), ("u1", (4,)), "<u4", "<u4"],
    "offsets": [0, 12, 16, 24, 48, 56, 68, 80, 84, 88, 92, 96, 108, 112, 124, 128, 132, 136, 140],
    "itemsize": 144})
CURSOR_NO_BLOCK = 0xFFFFFFFF  # AIC_CURSOR_NO_BLOCK: preceding_block_index of a cube outside the bounds

LINE_VERTEX_DTYPE = np.dtype([("position", "<f4", (3,)), ("color", "<f4", (4,))])  # aic_line_vertex: 28 bytes


def cursor_wireframe(cube, face_entered: int, face_selected: int, point_entered, distance_to_point: float, voxel_lo=(0, 0, 0), voxel_size=(1, 1, 1),
                     resolution: int = 1):
    """The cursor's line list (aic_cursor_wireframe; impl Wireframe for Cursor, cursor.rs:219-278): [2 n] LINE_VERTEX_DTYPE records, n = 12, 16, 24 or
    28. Faces are Face7 discriminants; voxel_lo / voxel_size / resolution are the hit block's voxels_bounds() and resolution. Host-only."""
    lib = load()
    lib.aic_cursor_wireframe.restype = C.c_int
    lib.aic_cursor_wireframe.argtypes = [C.POINTER(CursorDesc), C.c_void_p, C.POINTER(C.c_uint32)]
    d = CursorDesc()
    d.cube[:], d.point_entered[:], d.voxel_lo[:], d.voxel_size[:] = [int(v) for v in cube], [float(v) for v in point_entered], [int(v) for v in voxel_lo], [int(v) for v in voxel_size]
    d.face_entered, d.face_selected, d.distance_to_point, d.resolution = int(face_entered), int(face_selected), float(distance_to_point), int(resolution)
    out = np.zeros(2 * CURSOR_MAX_LINES, LINE_VERTEX_DTYPE)
    n = C.c_uint32(0)
    rc = lib.aic_cursor_wireframe(C.byref(d), out.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc != 0:
        raise AicError(rc, "aic_cursor_wireframe")
    return out[:2 * n.value].copy()


# aic_light_cube_info (32 bytes) and aic_light_ray (40 bytes): what aic_light_rays answers per cube and per pushed record
LIGHT_CUBE_INFO_DTYPE = np.dtype([("cube", "<i4", (3,)), ("result", "u1", (4,)), ("cost", "<u4"), ("n_rays", "<u4"), ("first_ray", "<u4"), ("flags", "<u4")])
LIGHT_RAY_DTYPE = np.dtype([("trigger_cube", "<i4", (3,)), ("value_cube", "<i4", (3,)), ("value", "u1", (4,)), ("light_from_struck_face", "<f4", (3,))])
LIGHT_RAYS_DEVICE = 1                           # AIC_LIGHT_RAYS_DEVICE: rays and lines are device pointers
LIGHT_CUBE_STORED, LIGHT_CUBE_OUTSIDE = 1, 2    # aic_light_cube_info.flags
LIGHT_RAYS_MAX_CUBES = 1 << 16
LIGHT_RAY_BOX_LINES, LIGHT_RAY_LINES = 12, 29   # lines of a cube's box; lines of one record (its value cube's box and the arrow's 17)


def light_rays_bound(maximum_distance: int) -> int:
    """The most records one cube can produce with this maximum_distance (aic_light_rays_bound), counted in the chart. Host-only."""
    lib = load()
    lib.aic_light_rays_bound.restype = C.c_uint32
    lib.aic_light_rays_bound.argtypes = [C.c_int32]
    return int(lib.aic_light_rays_bound(int(maximum_distance)))


def light_rays_wireframe(info, rays) -> np.ndarray:
    """The lines of one cube (aic_light_rays_wireframe; impl Wireframe for LightUpdateCubeInfo, light/debug.rs:50-95) from its LIGHT_CUBE_INFO_DTYPE
    record and its own n_rays LIGHT_RAY_DTYPE records: [2 * (12 + 29 n_rays)] LINE_VERTEX_DTYPE records. Host-only."""
    lib = load()
    lib.aic_light_rays_wireframe.restype = C.c_int
    lib.aic_light_rays_wireframe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    i = np.ascontiguousarray(info, LIGHT_CUBE_INFO_DTYPE).reshape(1)
    r = np.ascontiguousarray(rays, LIGHT_RAY_DTYPE).reshape(-1)
    if len(r) != int(i["n_rays"][0]):
        raise ValueError("light_rays_wireframe: info.n_rays records wanted")
    out = np.zeros(2 * (LIGHT_RAY_BOX_LINES + LIGHT_RAY_LINES * len(r)), LINE_VERTEX_DTYPE)
    n = C.c_uint32(0)
    rc = lib.aic_light_rays_wireframe(_ptr(i), _ptr(r) if len(r) else None, _ptr(out), C.byref(n))
    if rc != 0:
        raise AicError(rc, "aic_light_rays_wireframe")
    return out[:2 * n.value]


def text_geometry(nominal_size, cell=(9, 18, 1), origin_px=(5.0, 5.0)):
    """The info text's character grid and texture-coordinate transform for a viewport of `nominal_size` = (width, height) nominal pixels and a font
    `cell` = (cell_width, cell_height, cell_margin) (aic_text_geometry; character_texture_size, text.rs:20-52, and PostprocessUniforms::new,
    postprocess.rs:316-331): (cols, rows, scale [2] float32, origin [2] float32). Host-only: needs no device or context."""
    lib = load()
    lib.aic_text_geometry.restype = C.c_int
    lib.aic_text_geometry.argtypes = [C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_float), C.POINTER(C.c_float)]
    cols, rows, scale, origin, px = C.c_uint32(0), C.c_uint32(0), (C.c_float * 2)(), (C.c_float * 2)(), (C.c_double * 2)(float(origin_px[0]), float(origin_px[1]))
    rc = lib.aic_text_geometry(float(nominal_size[0]), float(nominal_size[1]), int(cell[0]), int(cell[1]), int(cell[2]), px, C.byref(cols), C.byref(rows), scale, origin)
    if rc != 0:
        raise AicError(rc, f"aic_text_geometry({tuple(nominal_size)}, {tuple(cell)})")
    return cols.value, rows.value, np.array(scale[:], np.float32), np.array(origin[:], np.float32)


def text_layout(text, cols: int, rows: int):
    """`text` -- a str, or bytes taken as UTF-8, malformed or not -- laid out in a rows x cols grid of character codes (aic_text_layout;
    render_text_to_character_texture, text.rs:56-73): (codes [rows][cols] uint8, (used columns, used rows)). Host-only."""
    lib = load()
    lib.aic_text_layout.restype = C.c_int
    lib.aic_text_layout.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    ok = 0 < cols <= 65535 and 0 < rows <= 65535
    codes = np.zeros((rows, cols) if ok else (1, 1), np.uint8)
    used = (C.c_uint32 * 2)()
    rc = lib.aic_text_layout(raw, len(raw), int(cols), int(rows), codes.ctypes.data_as(C.c_void_p), used)
    if rc != 0:
        raise AicError(rc, f"aic_text_layout(cols {cols}, rows {rows})")
    return codes, (used[0], used[1])


CELL_DTYPE = np.dtype([("glyph", "<u4"), ("fg", "<u4"), ("bg", "<u4")])  # aic_cell: 12 bytes


class CellsDesc(C.Structure):
    _fields_ = [("cols", C.c_uint32), ("rows", C.c_uint32), ("characters", C.c_int32), ("colors", C.c_int32), ("exposure", C.c_float),
                ("tone_mapping", C.c_int32), ("maximum_intensity", C.c_float), ("flags", C.c_uint32)]


class CellsInfo(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("n_cells", "n_full", "n_upper", "n_lower", "n_text", "n_space", "n_shade", "n_rising", "n_falling", "n_equal",
                                          "n_unequal", "n_names", "n_braille", "n_gray", "n_cube", "n_rgb")] + [("kernel_ms", C.c_float), ("reserved", C.c_uint32)]

    def counters(self) -> dict:
        """The branch counters by name, as tests/cells_ref.py counts them."""
        return {k: int(getattr(self, k)) for k, _ in self._fields_[1:16]}


class CellsText(C.Structure):
    _fields_ = [("names", C.POINTER(C.c_char_p) * 2), ("widths", C.POINTER(C.c_uint8) * 2), ("n_names", C.c_uint32 * 2), ("origin", C.c_uint16 * 2),
                ("reserved", C.c_uint32)]


def cells_geometry(cols: int, rows: int, characters: int):
    """TerminalOptions::viewport_from_terminal_size (aic_cells_geometry): ((width, height) of the framebuffer, (nominal width, height))."""
    w, h, nominal = C.c_uint32(), C.c_uint32(), (C.c_double * 2)()
    rc = load().aic_cells_geometry(int(cols), int(rows), int(characters), C.byref(w), C.byref(h), nominal)
    if rc != AIC_OK:
        raise AicError(rc, f"aic_cells_geometry({cols}, {rows}, characters {characters})")
    return (w.value, h.value), (nominal[0], nominal[1])


def cells_ansi(cells, names=None, widths=None, in_rect: bool = False, origin=(0, 0), capacity: Optional[int] = None) -> bytes:
    """write_frame as a byte stream (aic_cells_ansi). cells: [rows][cols] of CELL_DTYPE. names / widths: per layer (world, ui) a list of str (None
    entries allowed) / of column widths, or None. `capacity`: the buffer to offer (default: exactly what the stream needs)."""
    cells = np.ascontiguousarray(cells, CELL_DTYPE)
    rows, cols = cells.shape
    text = CellsText()
    keep = []
    for layer in (0, 1):
        table = names[layer] if names else None
        if table is not None:
            arr = (C.c_char_p * max(len(table), 1))(*[None if t is None else t.encode() for t in table])
            keep.append(arr)
            text.names[layer] = C.cast(arr, C.POINTER(C.c_char_p))
            text.n_names[layer] = len(table)
            if widths and widths[layer] is not None:
                wa = (C.c_uint8 * max(len(table), 1))(*[int(v) for v in widths[layer]])
                keep.append(wa)
                text.widths[layer] = C.cast(wa, C.POINTER(C.c_uint8))
    text.origin[0], text.origin[1] = int(origin[0]), int(origin[1])
    lib = load()
    flags = CELLS_ANSI_IN_RECT if in_rect else 0
    length = C.c_uint64()
    if capacity is None:
        lib.aic_cells_ansi(_ptr(cells) if cells.size else None, cols, rows, C.byref(text), flags, None, 0, C.byref(length))
        capacity = length.value
    buf = C.create_string_buffer(max(int(capacity), 1))
    rc = lib.aic_cells_ansi(_ptr(cells) if cells.size else None, cols, rows, C.byref(text), flags, buf, int(capacity), C.byref(length))
    if rc != AIC_OK:
        raise AicError(rc, f"aic_cells_ansi: the stream needs {length.value} bytes, capacity {capacity}")
    return buf.raw[:length.value]


PIXEL_AUX_DTYPE = np.dtype(
    [("hit", "<i4"), ("cube", "<i4", (3,)), ("voxel", "<i4", (3,)), ("resolution", "<i4"), ("face", "<i4"),
     ("block_index", "<i4"), ("cubes_traced", "<u4"), ("layer", "<u4"), ("t_distance", "<f8")],
    align=True,
)
RC_STEP_DTYPE = np.dtype([("cube", "<i4", (3,)), ("face", "<i4"), ("t_distance", "<f8"), ("intersection_point", "<f8", (3,))], align=True)

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Loads libaic_hip.so; raises if it has not been built (run `python __graft_entry__.py`)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc, gfx950)")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and libaic_hip.so is linked against /opt/rocm's. Loaded
        # after torch, this library binds to the copy already in the process; loaded BEFORE torch, the process ends up with two
        # runtimes and the second one to initialise finds no GPU ("No HIP GPUs are available" from torch.zeros(device="cuda") --
        # met by tests/test_gpu_light_update.py run on its own). A process that has torch gets it loaded first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(str(LIB_PATH))
        lib.aic_create.restype = C.c_void_p
        lib.aic_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
        lib.aic_destroy.argtypes = [C.c_void_p]
        lib.aic_destroy.restype = None
        lib.aic_last_error.restype = C.c_char_p
        lib.aic_last_error.argtypes = [C.c_void_p]
        lib.aic_stream.restype = C.c_void_p
        lib.aic_stream.argtypes = [C.c_void_p]
        lib.aic_partition_rows.restype = C.c_uint32
        lib.aic_partition_rows.argtypes = [C.c_uint32, C.POINTER(Partition)]
        lib.aic_upload_space.argtypes = [C.c_void_p, C.c_int, C.POINTER(SpaceDesc)]
        lib.aic_clear_space.argtypes = [C.c_void_p, C.c_int]
        lib.aic_compact.argtypes = [C.c_void_p, C.c_int]
        lib.aic_update_cubes.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.aic_update_light_volume.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_replace_block.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(BlockDesc), C.c_void_p, C.c_void_p]
        lib.aic_replace_blocks.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.aic_set_options.argtypes = [C.c_void_p, C.c_int, C.POINTER(Options)]
        lib.aic_set_depth_transform.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.aic_render.argtypes = [C.c_void_p, C.POINTER(FrameDesc), C.c_void_p, C.c_int, C.POINTER(FrameInfo)]
        lib.aic_render_submit.argtypes = [C.c_void_p, C.POINTER(FrameDesc), C.c_void_p, C.c_uint32]
        lib.aic_render_wait.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(FrameInfo)]
        lib.aic_render_submit_batch.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(FrameDesc), C.POINTER(C.c_void_p), C.c_uint32]
        lib.aic_render_wait_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(FrameInfo)]
        lib.aic_trace_patches.argtypes = [C.c_void_p, C.POINTER(FrameDesc), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FrameInfo)]
        lib.aic_trace_rays.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(FrameInfo)]
        lib.aic_trace_pixels.argtypes = [C.c_void_p, C.POINTER(FrameDesc), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(FrameInfo)]
        lib.aic_reproject_split.argtypes = [C.c_void_p, C.POINTER(ReprojectDesc), C.c_void_p, C.c_void_p, C.POINTER(ReprojectInfo)]
        lib.aic_pick_pixels.argtypes = [C.c_void_p, C.POINTER(PickDesc), C.c_void_p, C.c_void_p, C.POINTER(PickInfo)]
        lib.aic_pick_stale.argtypes = [C.c_void_p, C.POINTER(StaleDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StaleInfo)]
        lib.aic_light_changed_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
        lib.aic_light_changed_take.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.aic_pick_stale_cubes.argtypes = [C.c_void_p, C.POINTER(StaleCubesDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StaleCubesInfo)]
        lib.aic_probe_stale_cube_rects.argtypes = [C.c_void_p, C.POINTER(StaleCubesDesc), C.c_void_p]
        lib.aic_find_block_cubes.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(BlockCubesInfo)]
        lib.aic_replace_cube_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(BlockCubesInfo)]
        lib.aic_copy_cube_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.aic_update_light_volume_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_pick_stale_blocks.argtypes = [C.c_void_p, C.POINTER(StaleBlocksDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StaleBlocksInfo)]
        lib.aic_present_split.argtypes = [C.c_void_p, C.POINTER(PresentDesc), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PresentInfo)]
        lib.aic_present_split_lines.argtypes = [C.c_void_p, C.POINTER(PresentDesc), C.POINTER(LinesDesc), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PresentInfo),
                                                C.POINTER(LinesInfo)]
        lib.aic_set_text_font.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.aic_present_split_text.argtypes = [C.c_void_p, C.POINTER(PresentDesc), C.POINTER(LinesDesc), C.POINTER(TextDesc), C.c_void_p, C.c_void_p, C.c_int,
                                               C.POINTER(PresentInfo), C.POINTER(LinesInfo)]
        lib.aic_export_split.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ExportInfo)]
        lib.aic_sample_luminance.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.aic_cursor_raycast.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_double, C.c_uint32, C.c_void_p]
        lib.aic_light_rays.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.aic_cells_geometry.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        lib.aic_cells_ansi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(CellsText), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.aic_image_cells.argtypes = [C.c_void_p, C.POINTER(CellsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CellsInfo)]
        lib.aic_render_cells.argtypes = [C.c_void_p, C.POINTER(FrameDesc), C.POINTER(CellsDesc), C.c_void_p, C.c_int, C.POINTER(FrameInfo), C.POINTER(CellsInfo)]
        lib.aic_export_size.restype = C.c_int
        lib.aic_export_size.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_uint32)]
        lib.aic_assemble_strips.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.aic_assemble_strips_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.aic_read_aux.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.aic_synchronize.argtypes = [C.c_void_p]
        lib.aic_wait_event.argtypes = [C.c_void_p, C.c_void_p]
        lib.aic_stream_wait_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        lib.aic_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
        lib.aic_probe_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        lib.aic_probe_light_lut.argtypes = [C.c_void_p, C.c_void_p]
        lib.aic_probe_powf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.aic_probe_expf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.aic_probe_bloom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.POINTER(Options), C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint32 * 2)]
        lib.aic_evaluate_light.argtypes = [C.c_void_p, C.c_int, C.POINTER(LightParams), C.POINTER(LightInfo)]
        lib.aic_evaluate_light_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(LightParams)]
        lib.aic_evaluate_light_wait.argtypes = [C.c_void_p, C.c_int, C.POINTER(LightInfo)]
        lib.aic_evaluate_light_poll.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        lib.aic_read_light_volume.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_read_light_cubes.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.aic_light_cubes_changed.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int]
        lib.aic_probe_derived.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.aic_probe_log2f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.aic_probe_cube_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        assert C.sizeof(BlockDesc) == 48
        _lib = lib
    return _lib


def packed_light_scalar_in(value: float) -> int:
    """PackedLight::scalar_in (all-is-cubes/src/space/light/data.rs:214-218)."""
    v = np.float32(value)
    if not v > 0:
        return 0
    x = float(np.float32(np.float32(np.log2(v)) * np.float32(10.0)) + np.float32(144.0))
    x = float(np.float32(x))
    r = math.floor(abs(x) + 0.5) * (1 if x >= 0 else -1)  # f32::round: half away from zero
    return int(min(max(r, 0), 255))


def block_sky_texels(sky_kind: int, sky: np.ndarray) -> np.ndarray:
    """Sky::for_blocks (all-is-cubes/src/space/sky.rs:45-82) as 7 texels: nx ny nz px py pz mean."""
    sky = np.asarray(sky, np.float32).reshape(8, 3)
    out = np.zeros((7, 4), np.uint8)
    out[:, 3] = 255  # LightStatus::Visible

    def some(rgb):
        return [packed_light_scalar_in(float(c)) for c in rgb]

    if sky_kind == 0:
        out[:, 0:3] = some(sky[0])
        return out
    # images of +X,+Y,+Z under Face::rotation_from_nz (face.rs:395-404)
    bases = {
        0: ((0, 1, 0), (0, 0, 1), (1, 0, 0)),  # NX RYZX
        1: ((0, 0, 1), (1, 0, 0), (0, 1, 0)),  # NY RZXY
        2: ((1, 0, 0), (0, 1, 0), (0, 0, 1)),  # NZ RXYZ
        3: ((0, -1, 0), (0, 0, 1), (-1, 0, 0)),  # PX RyZx
        4: ((0, 0, 1), (-1, 0, 0), (0, -1, 0)),  # PY RZxy
        5: ((1, 0, 0), (0, -1, 0), (0, 0, -1)),  # PZ RXyz
    }
    pts = [(-1, -1, -1), (-1, 1, -1), (1, -1, -1), (1, 1, -1)]
    for f in range(6):
        bx, by, bz = (np.array(v) for v in bases[f])
        acc = np.zeros(3, np.float32)
        for p in pts:
            d = p[0] * bx + p[1] * by + p[2] * bz
            idx = ((1 if d[0] >= 0 else 0) << 2) + ((1 if d[1] >= 0 else 0) << 1) + (1 if d[2] >= 0 else 0)
            acc = (acc + sky[idx]).astype(np.float32)
        out[f, 0:3] = some(acc * np.float32(0.25))
    acc = np.zeros(3, np.float32)
    for k in range(8):
        acc = (acc + sky[k]).astype(np.float32)
    out[6, 0:3] = some(acc * np.float32(1.0 / 8.0))
    return out


def make_options(fog=1, transparency=1, threshold=0.5, lighting=3, bounce_samples=0, antialiasing=0, debug_pixel_cost=False,
                 tone_mapping=0, maximum_intensity=float("inf"), bloom_intensity=0.125, view_distance=200.0) -> Options:
    """Defaults = GraphicsOptions::default() (camera/graphics_options.rs:256-280)."""
    o = Options()
    o.fog, o.transparency, o.threshold, o.lighting = fog, transparency, threshold, lighting
    o.bounce_samples, o.antialiasing, o.debug_pixel_cost = bounce_samples, antialiasing, int(debug_pixel_cost)
    o.tone_mapping, o.maximum_intensity, o.bloom_intensity = tone_mapping, maximum_intensity, bloom_intensity
    o.view_distance = min(max(view_distance, 1.0), 10000.0)  # GraphicsOptions::repair
    return o


def unaltered_colors(**kw) -> Options:
    """GraphicsOptions::UNALTERED_COLORS (graphics_options.rs:168-190)."""
    base = dict(fog=0, lighting=0, transparency=1, bloom_intensity=0.0)
    base.update(kw)
    return make_options(**base)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else a.ctypes.data


def device_array_ptr(a, dtypes, count: int, what: str, device_index: Optional[int] = None) -> int:
    """The address of an array in device memory, for the calls that take one (replace_cube_grid, copy_cube_grid, update_light_volume_device): a raw
    pointer (an int) as it is, or a torch tensor -- checked here, before the call: its dtype is one of `dtypes` (names of torch dtypes of one element
    size, e.g. ("uint16", "int16"): the bits are taken as they are), it has `count` elements, is contiguous and lives on the GPU `device_index`
    (None: any GPU; the library looks at the pointer itself as well)."""
    if a is None:
        return 0
    if isinstance(a, (int, np.integer)):
        return int(a)
    if not (hasattr(a, "data_ptr") and hasattr(a, "is_contiguous")):
        raise TypeError(f"{what}: a torch tensor on the device or a raw device pointer, not {type(a).__name__}")
    name = str(a.dtype).replace("torch.", "")
    if name not in dtypes:
        raise ValueError(f"{what}: dtype {name}, not {' or '.join(dtypes)}")
    if int(a.numel()) != int(count):
        raise ValueError(f"{what}: {int(a.numel())} elements, not the layer's {int(count)}")
    if not a.is_contiguous():
        raise ValueError(f"{what}: the tensor is not contiguous")
    if a.device.type != "cuda":
        raise ValueError(f"{what}: the tensor is on {a.device}, not in device memory")
    if device_index is not None and a.device.index != device_index:
        raise ValueError(f"{what}: the tensor is on device {a.device.index}, the context on device {device_index}")
    return int(a.data_ptr())


class Context:
    """One device-resident renderer state = `RtRenderer` minus cameras."""

    def __init__(self, device_id: int = -1):
        self._lib = load()
        self._device_id = int(device_id) if device_id >= 0 else None  # (None: whatever device was current; the library checks device pointers itself)
        self._layer_cubes = {}  # layer -> cubes of the space uploaded through this object: what a device array is measured against
        st = C.c_int(0)
        self._h = self._lib.aic_create(device_id, C.byref(st))
        if not self._h:
            raise AicError(st.value, "aic_create failed (no usable MI355X / HIP device?)")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.aic_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != AIC_OK:
            raise AicError(rc, self._lib.aic_last_error(self._h).decode())

    @property
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self._lib.aic_device_name(self._h, buf, 256))
        return buf.value.decode()

    @property
    def stream(self) -> int:
        return int(self._lib.aic_stream(self._h) or 0)

    # -- scene ---------------------------------------------------------------------------
    @staticmethod
    def _space_desc(flat_space):
        """(SpaceDesc, keep-alive) for aic_upload_space / aic_multi_upload_space."""
        p = flat_space.pack() if hasattr(flat_space, "pack") else flat_space
        d = SpaceDesc()
        d.lo[:] = [int(v) for v in p.lo]
        d.size[:] = [int(v) for v in p.size]
        d.block_index = _ptr(p.block_index)
        d.light = _ptr(p.light)
        d.n_blocks = len(p.blocks)
        d.blocks = _ptr(p.blocks)
        d.voxels = _ptr(p.voxels)
        d.n_voxels = p.voxels.size
        d.palette = _ptr(p.palette)
        d.n_palette = len(p.palette)
        d.sky_kind = p.sky_kind
        for i in range(8):
            for j in range(3):
                d.sky[i][j] = float(p.sky[i, j])
        bs = block_sky_texels(p.sky_kind, p.sky)
        for i in range(7):
            for j in range(4):
                d.block_sky[i][j] = int(bs[i, j])
        return d, p

    def upload_space(self, layer: int, flat_space) -> None:
        d, _keep = self._space_desc(flat_space)
        self._check(self._lib.aic_upload_space(self._h, layer, C.byref(d)))
        self._layer_cubes[int(layer)] = int(d.size[0]) * int(d.size[1]) * int(d.size[2])

    def clear_space(self, layer: int) -> None:
        self._check(self._lib.aic_clear_space(self._h, layer))
        self._layer_cubes.pop(int(layer), None)

    def update_cubes(self, layer: int, xyz, block_index=None, light=None) -> None:
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        bi = None if block_index is None else np.ascontiguousarray(block_index, np.uint16)
        lt = None if light is None else np.ascontiguousarray(light, np.uint8).reshape(-1, 4)
        self._check(self._lib.aic_update_cubes(self._h, layer, len(xyz), _ptr(xyz), _ptr(bi), _ptr(lt)))

    def update_light_volume(self, layer: int, light: np.ndarray) -> None:
        lt = np.ascontiguousarray(light, np.uint8)
        self._check(self._lib.aic_update_light_volume(self._h, layer, _ptr(lt)))

    def _device_arrays(self, layer: int, index_array, light_array, names):
        """The addresses of a layer's index array and light array in device memory (device_array_ptr's checks, against the space uploaded here)."""
        n = self._layer_cubes.get(int(layer))
        if n is None:
            raise AicError(1, f"no space uploaded for layer {layer} through this context")
        return (device_array_ptr(index_array, ("uint16", "int16"), n, names[0], self._device_id),
                device_array_ptr(light_array, ("uint8",), 4 * n, names[1], self._device_id))

    def replace_cube_grid(self, layer: int, block_index, light=None, capacity: int = 4096):
        """The block index of every cube of `layer` from device memory (aic_replace_cube_grid): `block_index` is a torch tensor of the layer's
        cubes as uint16 (or int16, bits as they are) on the context's device, Z-major plain indices, or a raw device pointer; `light`, if given,
        cubes x 4 uint8 texels. Returns (boxes [n_written, 6] int32 {lo, hi exclusive} -- the runs of changed cubes along z, as find_block_cubes
        gives them, ready for pick_stale_cubes; the one box `bounds` when there are more runs than `capacity` --, info as a dict: n_cubes, n_runs,
        bounds, n_written, merged, kernel_ms). The tensors must be complete (their stream synchronised, or ordered with wait_event) and are free
        again on return."""
        bi, lt = self._device_arrays(layer, block_index, light, ("block_index", "light"))
        out = np.zeros((max(int(capacity), 1), 6), np.int32)
        info = BlockCubesInfo()
        self._check(self._lib.aic_replace_cube_grid(self._h, int(layer), C.c_void_p(bi or None), C.c_void_p(lt or None), int(capacity),
                                                    C.c_void_p(out.ctypes.data if capacity else None), C.byref(info)))
        return out[:info.n_written].copy(), dict(n_cubes=int(info.n_cubes), n_runs=int(info.n_runs), bounds=[int(v) for v in info.bounds],
                                                 n_written=int(info.n_written), merged=int(info.merged), kernel_ms=float(info.kernel_ms))

    def copy_cube_grid(self, layer: int, out=None, light_out=None) -> None:
        """The layer's grid into device memory as plain indices, tags stripped (`out`: uint16 / int16, one per cube), and its published light
        volume (`light_out`: cubes x 4 uint8) (aic_copy_cube_grid): how a device simulation starts from an uploaded scene. Tensors or raw pointers."""
        o, lo = self._device_arrays(layer, out, light_out, ("out", "light_out"))
        self._check(self._lib.aic_copy_cube_grid(self._h, int(layer), C.c_void_p(o or None), C.c_void_p(lo or None)))

    def update_light_volume_device(self, layer: int, light) -> None:
        """update_light_volume with the texels in device memory (aic_update_light_volume_device): cubes x 4 uint8, a tensor or a raw pointer."""
        _, lt = self._device_arrays(layer, None, light, ("", "light"))
        self._check(self._lib.aic_update_light_volume_device(self._h, int(layer), C.c_void_p(lt or None)))

    def replace_block(self, layer: int, index: int, block) -> None:
        from . import flat

        d = BlockDesc()
        d.resolution = block.resolution
        d.vlo[:] = list(block.vlo)
        d.vsize[:] = list(block.voxels.shape)
        d.pal_len = len(block.palette)
        d.flags = flat.block_flags(block)
        vox = np.ascontiguousarray(block.voxels, np.uint16)
        pal = flat.block_palette(block)
        self._check(self._lib.aic_replace_block(self._h, layer, index, C.byref(d), _ptr(vox), _ptr(pal)))

    def render_orthographic(self, layer: int = LAYER_WORLD, resolution: int = 32):
        """raytracer::ortho::render_orthographic of the layer's space: dict(rgba8 [h,w,4], info)."""
        f = self._lib.aic_render_orthographic
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
        w, h = C.c_uint32(0), C.c_uint32(0)
        self._check(f(self._h, layer, resolution, None, 0, C.byref(w), C.byref(h), None))
        out = np.zeros((h.value, w.value, 4), np.uint8)
        info = FrameInfo()
        self._check(f(self._h, layer, resolution, _ptr(out), 0, C.byref(w), C.byref(h), C.byref(info)))
        return {"rgba8": out, "info": info}

    def compact(self, layer: int) -> None:
        self._check(self._lib.aic_compact(self._h, C.c_int(layer)))

    def replace_blocks(self, layer: int, items) -> None:
        """`items`: list of (index, flat.BlockDef) -- a batch of BlockEvaluation changes under one synchronisation."""
        from . import flat

        n = len(items)
        idx = np.ascontiguousarray([i for i, _ in items], np.uint32)
        descs = (BlockDesc * max(n, 1))()
        keep, vp, pp = [], (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
        for k, (_, block) in enumerate(items):
            d = descs[k]
            d.resolution = block.resolution
            d.vlo[:] = list(block.vlo)
            d.vsize[:] = list(block.voxels.shape)
            d.pal_len = len(block.palette)
            d.flags = flat.block_flags(block)
            vox = np.ascontiguousarray(block.voxels, np.uint16)
            pal = flat.block_palette(block)
            keep += [vox, pal]
            vp[k], pp[k] = vox.ctypes.data, pal.ctypes.data
        self._check(self._lib.aic_replace_blocks(self._h, layer, n, _ptr(idx), C.cast(descs, C.c_void_p), C.cast(vp, C.c_void_p), C.cast(pp, C.c_void_p)))

    def set_options(self, layer: int, options: Options) -> None:
        self._check(self._lib.aic_set_options(self._h, layer, C.byref(options)))

    def set_depth_transform(self, zw) -> None:
        """aic_set_depth_transform: zw = (m33, m43, m34, m44) of the depth transform FRAME_OUT_SPLIT frames apply; (1, 0, 0, 1) = linear depth."""
        self._check(self._lib.aic_set_depth_transform(self._h, (C.c_double * 4)(*[float(v) for v in zw])))

    # -- drawing ---------------------------------------------------------------------------
    @staticmethod
    def make_frame(width, height, world_inv=None, ui_inv=None, exposure=1.0, ui_exposure=1.0, backdrop=(0, 0, 0, 0),
                   partition=None, flags=0, tuning=0) -> FrameDesc:
        f = FrameDesc()
        f.width, f.height = int(width), int(height)
        ident = np.eye(4).reshape(16)
        w = ident if world_inv is None else np.ascontiguousarray(world_inv, np.float64).reshape(16)
        u = ident if ui_inv is None else np.ascontiguousarray(ui_inv, np.float64).reshape(16)
        f.world.inverse_projection_view[:] = [float(v) for v in w]
        f.ui.inverse_projection_view[:] = [float(v) for v in u]
        f.world.exposure, f.ui.exposure = exposure, ui_exposure
        f.backdrop[:] = [float(v) for v in backdrop]
        if partition is not None:
            f.partition.strip_rows, f.partition.n_parts, f.partition.part = (int(v) for v in partition)
        f.flags = flags
        f.tuning = int(tuning)
        return f

    def partition_rows(self, height: int, partition) -> int:
        p = Partition(int(partition[0]), int(partition[1]), int(partition[2]), 0)
        return int(self._lib.aic_partition_rows(height, C.byref(p)))

    def render(self, frame: FrameDesc, want_aux: bool = False, counters: bool = False):
        """Returns dict(rgba8 [rows,w,4], info FrameInfo, aux or None); for a FRAME_OUT_SPLIT frame dict(color_f16 [rows,w,4] float16, depth [rows,w]
        float32, info, aux or None). `frame` is left as it was given (until round 6 want_aux / counters
        stayed set in it, and a later plain render of the same object quietly ran the recording variant again)."""
        keep_flags = frame.flags
        if want_aux:
            frame.flags |= FRAME_AUX
        if counters:
            frame.flags |= FRAME_COUNTERS
        rows = int(self._lib.aic_partition_rows(frame.height, C.byref(frame.partition)))
        floats = bool(frame.flags & (FRAME_OUT_LINEAR | FRAME_OUT_COLORBUF))  # 16-byte float pixels instead of RGBA8
        split = bool(frame.flags & FRAME_OUT_SPLIT) and not floats
        out = np.zeros(rows * frame.width * 3, np.uint32) if split else np.zeros((rows, frame.width, 4), np.float32 if floats else np.uint8)
        info = FrameInfo()
        try:
            self._check(self._lib.aic_render(self._h, C.byref(frame), _ptr(out), 0, C.byref(info)))
        finally:
            frame.flags = keep_flags
        aux = None
        if want_aux:
            aux = np.zeros((rows, frame.width), PIXEL_AUX_DTYPE)
            if aux.size:
                self._check(self._lib.aic_read_aux(self._h, _ptr(aux), aux.size))
        if split:
            return {**split_planes(out, rows, frame.width), "info": info, "aux": aux}
        return {"rgba8": out, "info": info, "aux": aux}

    def render_to_device(self, frame: FrameDesc, device_ptr: int) -> FrameInfo:
        """Leaves the RGBA8 rows in HBM at `device_ptr` (e.g. a torch tensor's data_ptr())."""
        info = FrameInfo()
        self._check(self._lib.aic_render(self._h, C.byref(frame), C.c_void_p(device_ptr), 1, C.byref(info)))
        return info

    def trace_patches(self, frame: FrameDesc, rects, want_aux: bool = False):
        """RtScene::trace_patch for a batch of NDC rectangles [n,4] = (min.x, min.y, max.x, max.y)."""
        r = np.ascontiguousarray(rects, np.float64).reshape(-1, 4)
        out = np.zeros((len(r), 4), np.float32 if frame.flags & (FRAME_OUT_LINEAR | FRAME_OUT_COLORBUF) else np.uint8)
        aux = np.zeros(len(r), PIXEL_AUX_DTYPE) if want_aux else None
        info = FrameInfo()
        self._check(self._lib.aic_trace_patches(self._h, C.byref(frame), len(r), _ptr(r), _ptr(out), _ptr(aux), C.byref(info)))
        return {"rgba8": out, "aux": aux, "info": info}

    def trace_rays(self, layer: int, rays, include_sky: bool = True, flags: int = 0, exposure: float = 1.0, want_aux: bool = False):
        """SpaceRaytracer::trace_ray for a batch of world-space rays [n,6] = (origin xyz, direction xyz) against the layer's space (aic_trace_rays).
        `flags`: FRAME_OUT_COLORBUF / FRAME_OUT_LINEAR (float [n,4]; neither: RGBA8 [n,4]), FRAME_COUNTERS. Returns dict(rgba8, aux or None, info)."""
        r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        flags = (int(flags) & ~RAYS_DEVICE) | (0 if include_sky else RAYS_NO_SKY)
        out = np.zeros((len(r), 4), np.float32 if flags & (FRAME_OUT_LINEAR | FRAME_OUT_COLORBUF) else np.uint8)
        aux = np.zeros(len(r), PIXEL_AUX_DTYPE) if want_aux else None
        info = FrameInfo()
        self._check(self._lib.aic_trace_rays(self._h, int(layer), len(r), _ptr(r), flags, float(exposure), _ptr(out), _ptr(aux), C.byref(info)))
        return {"rgba8": out, "aux": aux, "info": info}

    def trace_rays_device(self, layer: int, n: int, rays_ptr: int, out_ptr: int, aux_ptr: int = 0, include_sky: bool = True, flags: int = 0,
                          exposure: float = 1.0) -> FrameInfo:
        """The same with the rays ([n,6] f64), the results and (aux_ptr != 0) the [n] first-hit records in HBM on the context's device, e.g. torch tensors'
        data_ptr(): no staging copy, no read-back (AIC_RAYS_DEVICE). Returns once the batch is done."""
        flags = int(flags) | RAYS_DEVICE | (0 if include_sky else RAYS_NO_SKY)
        info = FrameInfo()
        self._check(self._lib.aic_trace_rays(self._h, int(layer), int(n), C.c_void_p(rays_ptr), flags, float(exposure), C.c_void_p(out_ptr),
                                             C.c_void_p(aux_ptr or None), C.byref(info)))
        return info

    def sample_luminance(self, layer: int, rays, max_steps: int) -> np.ndarray:
        """The luminance each of the rays [n,6] = (origin xyz, direction xyz) sees in the layer's space (aic_sample_luminance; the sampling loop of
        character::exposure::State::step, exposure.rs:91-128): float32 [n]. max_steps = 2 * maximum_distance, 0 for LightPhysics::None. Legal with
        frames in flight."""
        r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.zeros(len(r), np.float32)
        self._check(self._lib.aic_sample_luminance(self._h, int(layer), len(r), _ptr(r), int(max_steps), 0, _ptr(out)))
        return out

    def sample_luminance_device(self, layer: int, n: int, rays_ptr: int, max_steps: int, out_ptr: int) -> None:
        """The same with the rays ([n,6] f64) and the samples ([n] f32) in HBM on the context's device (AIC_RAYS_DEVICE): no staging, no read-back.
        Returns once the samples are there."""
        self._check(self._lib.aic_sample_luminance(self._h, int(layer), int(n), C.c_void_p(rays_ptr or None), int(max_steps), RAYS_DEVICE,
                                                   C.c_void_p(out_ptr or None)))

    def cursor_raycast(self, layer: int, rays, maximum_distance: float) -> np.ndarray:
        """cursor_raycast (cursor.rs:26-107) of each of the rays [n,6] = (origin xyz, direction xyz) against the layer's space, no further than
        maximum_distance (inf is legal): [n] CURSOR_HIT_DTYPE records (aic_cursor_raycast), all zero where the reference returns None. Legal with
        frames in flight."""
        r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.zeros(len(r), CURSOR_HIT_DTYPE)
        self._check(self._lib.aic_cursor_raycast(self._h, int(layer), len(r), _ptr(r), float(maximum_distance), 0, _ptr(out)))
        return out

    def cursor_raycast_device(self, layer: int, n: int, rays_ptr: int, maximum_distance: float, out_ptr: int) -> None:
        """The same with the rays ([n,6] f64) and the records ([n] of 144 bytes) in HBM on the context's device (AIC_RAYS_DEVICE), both at 8-byte
        boundaries: no staging, no read-back. Returns once the records are there."""
        self._check(self._lib.aic_cursor_raycast(self._h, int(layer), int(n), C.c_void_p(rays_ptr or None), float(maximum_distance), RAYS_DEVICE,
                                                 C.c_void_p(out_ptr or None)))

    def light_rays(self, layer: int, cubes, maximum_distance: int, capacity=None, want_lines: bool = True):
        """Space::compute_light::<LightUpdateCubeInfo> of each of the cubes [n,3] against the layer's published light volume (aic_light_rays): returns
        (infos [n] LIGHT_CUBE_INFO_DTYPE, rays LIGHT_RAY_DTYPE, lines [2 * n_lines] LINE_VERTEX_DTYPE or None, totals (rays, lines)). capacity None
        asks twice: once for the totals alone, then with room for exactly what the batch produces (the call stages a host list at the size it is given, and
        n * light_rays_bound is far more than a batch needs). rays and lines hold what was stored. Legal with frames in flight."""
        cu = np.ascontiguousarray(cubes, np.int32).reshape(-1, 3)
        n = len(cu)
        if capacity is None and n:
            first = np.zeros(2, np.uint64)
            self._check(self._lib.aic_light_rays(self._h, int(layer), n, _ptr(cu), int(maximum_distance), 0, 0, None, None, None, _ptr(first)))
            capacity = int(first[0])
        cap = int(capacity or 0)
        infos = np.zeros(n, LIGHT_CUBE_INFO_DTYPE)
        rays = np.zeros(max(cap, 1), LIGHT_RAY_DTYPE)
        lines = np.zeros(2 * (LIGHT_RAY_BOX_LINES * n + LIGHT_RAY_LINES * cap) + 2, LINE_VERTEX_DTYPE) if want_lines else None
        totals = np.zeros(2, np.uint64)
        self._check(self._lib.aic_light_rays(self._h, int(layer), n, _ptr(cu) if n else None, int(maximum_distance), 0, cap, _ptr(infos), _ptr(rays),
                                             _ptr(lines) if want_lines else None, _ptr(totals)))
        stored = infos[(infos["flags"] & LIGHT_CUBE_STORED) != 0]
        n_rays = int(stored["n_rays"].sum())
        n_lines = LIGHT_RAY_BOX_LINES * len(stored) + LIGHT_RAY_LINES * n_rays
        return infos, rays[:n_rays], (lines[:2 * n_lines] if want_lines else None), (int(totals[0]), int(totals[1]))

    def light_rays_device(self, layer: int, cubes, maximum_distance: int, capacity: int, rays_ptr: int, lines_ptr: int):
        """The same with the records ([capacity] of 40 bytes) and the lines ([2 * (12 n + 29 capacity)] vertices of 28 bytes) in HBM on the context's
        device (AIC_LIGHT_RAYS_DEVICE), either pointer 0 for none: nothing of them is staged or read back, and present_split_lines takes the lines as
        they stand. Returns (infos, totals)."""
        cu = np.ascontiguousarray(cubes, np.int32).reshape(-1, 3)
        infos = np.zeros(len(cu), LIGHT_CUBE_INFO_DTYPE)
        totals = np.zeros(2, np.uint64)
        self._check(self._lib.aic_light_rays(self._h, int(layer), len(cu), _ptr(cu) if len(cu) else None, int(maximum_distance), LIGHT_RAYS_DEVICE, int(capacity),
                                             _ptr(infos), C.c_void_p(rays_ptr or None), C.c_void_p(lines_ptr or None), _ptr(totals)))
        return infos, (int(totals[0]), int(totals[1]))

    def trace_pixels(self, frame: FrameDesc, pixels, want_aux: bool = False):
        """The listed pixels of `frame` (indices y * width + x, host memory), each traced exactly as render() traces it, results in list order
        (aic_trace_pixels, compact mode). Returns dict(rgba8 [n,4] uint8 or float32 by frame.flags, aux or None, info); for a FRAME_OUT_SPLIT frame
        dict(color_f16 [n,4] float16, depth [n] float32, aux, info)."""
        px = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        n = len(px)
        floats = bool(frame.flags & (FRAME_OUT_LINEAR | FRAME_OUT_COLORBUF))
        split = bool(frame.flags & FRAME_OUT_SPLIT) and not floats
        out = np.zeros(n * 3, np.uint32) if split else np.zeros((n, 4), np.float32 if floats else np.uint8)
        aux = np.zeros(n, PIXEL_AUX_DTYPE) if want_aux else None
        info = FrameInfo()
        self._check(self._lib.aic_trace_pixels(self._h, C.byref(frame), n, _ptr(px), 0, _ptr(out), _ptr(aux), C.byref(info)))
        if split:
            planes = split_planes(out, 1, n)
            return {"color_f16": planes["color_f16"].reshape(n, 4), "depth": planes["depth"].reshape(n), "aux": aux, "info": info}
        return {"rgba8": out, "aux": aux, "info": info}

    def trace_pixels_device(self, frame: FrameDesc, n: int, pixels_ptr: int, out_ptr: int, aux_ptr: int = 0, in_place: bool = False) -> FrameInfo:
        """The same with the list ([n] uint32), the results and (aux_ptr != 0) the [n] first-hit records in HBM on the context's device, e.g. torch
        tensors' data_ptr() (AIC_PIXELS_DEVICE). in_place: `out_ptr` is a whole frame of frame.width x frame.height as render_to_device leaves it (Split:
        the depth plane at byte offset width * height * 8); result i goes to pixel pixels[i] and every other texel stays (AIC_PIXELS_IN_PLACE) -- the
        resident textures of raytrace_to_texture's incremental loop. Returns once the batch is done."""
        mode = PIXELS_DEVICE | (PIXELS_IN_PLACE if in_place else 0)
        info = FrameInfo()
        self._check(self._lib.aic_trace_pixels(self._h, C.byref(frame), int(n), C.c_void_p(pixels_ptr or None), mode, C.c_void_p(out_ptr or None),
                                               C.c_void_p(aux_ptr or None), C.byref(info)))
        return info

    def reproject_split(self, width: int, height: int, matrix, ipzw, src_ptr: int, dst_ptr: int, flags: int = 0) -> ReprojectInfo:
        """A resident Split frame drawn into a new camera and gap-filled (aic_reproject_split). `src_ptr` and `dst_ptr` are whole Split frames of
        width x height in HBM on the context's device (the depth plane at byte offset width * height * 8) that do not overlap; `matrix` = the 16 floats of
        ReprojectionUniforms.reprojection_matrix, column-major ([c*4+r]; clip_new = M clip_old); `ipzw` = {ipz.z, ipw.z, ipz.w, ipw.w} of the current
        camera's inverse projection; flags: REPROJECT_KEEP_SPLATS. Returns once dst is written."""
        d = ReprojectDesc()
        d.width, d.height, d.flags = int(width), int(height), int(flags)
        d.reprojection[:] = [float(v) for v in np.asarray(matrix, np.float32).reshape(16)]
        d.inverse_projection_zw[:] = [float(v) for v in np.asarray(ipzw, np.float32).reshape(4)]
        info = ReprojectInfo()
        self._check(self._lib.aic_reproject_split(self._h, C.byref(d), C.c_void_p(src_ptr or None), C.c_void_p(dst_ptr or None), C.byref(info)))
        return info

    def pick_pixels(self, width: int, height: int, n: int, order_ptr: int, out_ptr: int, cursor: int = 0, max_unknown: int = 0, skip_unknown: int = 0,
                    flags: int = 0) -> PickInfo:
        """The next `n` pixel indices of a width x height frame written to `out_ptr` ([n] uint32 in HBM on the context's device), ready for
        trace_pixels_device(..., in_place=True) (aic_pick_pixels). `order_ptr`: pixel_order()'s order resident on the device ([width * height] uint32),
        or 0: row-major. The list holds first up to `max_unknown` of the pixels the context's last reproject_split of this size knows nothing about
        (the texels of its splat image with !(alpha > -0.5)), in the order's ranks, past the first `skip_unknown` of them; then the picker's picks
        `cursor`, `cursor` + 1, ... With max_unknown = 0 it is PixelPicker's sequence and the reprojection is not looked at. Returns once the list is
        written; the info's next_cursor and n_from_unknown are what the next call's cursor and skip_unknown advance by."""
        d = PickDesc()
        d.width, d.height, d.n, d.max_unknown = int(width), int(height), int(n), int(max_unknown)
        d.skip_unknown, d.cursor, d.flags = int(skip_unknown), int(cursor), int(flags)
        info = PickInfo()
        self._check(self._lib.aic_pick_pixels(self._h, C.byref(d), C.c_void_p(order_ptr or None), C.c_void_p(out_ptr or None), C.byref(info)))
        return info

    def pick_stale(self, width: int, height: int, n: int, rects, src_ptr: int, order_ptr: int, out_ptr: int, cursor: int = 0, max_stale: int = 0,
                   skip_stale: int = 0, flags: int = 0) -> StaleInfo:
        """pick_pixels with the stale pixels of the resident Split frame `src_ptr` first (aic_pick_stale): the pixels inside at least one of `rects`
        (stale_rects()'s records, at most STALE_MAX_RECTS) that does not keep them out -- with STALE_DEPTH_TEST a rectangle keeps out an opaque world
        pixel whose depth is below its dmin; without it none does and the frame is not read. Up to `max_stale` of them, in the order's ranks, past the
        first `skip_stale`; then the picker's picks `cursor`, `cursor` + 1, ... Returns once the list is written; the info's next_cursor and
        n_from_stale are what the next call's cursor and skip_stale advance by."""
        r = np.ascontiguousarray(np.asarray(rects, STALE_RECT_DTYPE).reshape(-1))
        d = StaleDesc()
        d.width, d.height, d.n, d.max_stale = int(width), int(height), int(n), int(max_stale)
        d.skip_stale, d.cursor, d.n_rects, d.flags = int(skip_stale), int(cursor), len(r), int(flags)
        d.rects = r.ctypes.data if len(r) else None
        info = StaleInfo()
        self._check(self._lib.aic_pick_stale(self._h, C.byref(d), C.c_void_p(src_ptr or None), C.c_void_p(order_ptr or None), C.c_void_p(out_ptr or None),
                                             C.byref(info)))
        return info

    def light_changed(self, layer: int, take: bool = True):
        """The cubes of `layer` whose light texel the updater changed since the baseline (aic_light_changed_count / _take): (xyz [n, 3] int32 ascending
        in the volume's cube index, bounds [6] int32 {lo, hi exclusive}; all 0 when n = 0). With `take` the baseline becomes the current volume -- and a
        submitted update is ended and published first; without it nothing is consumed, no update is waited for, and the answer is (n, bounds)."""
        n = C.c_uint64(0)
        bounds = np.zeros(6, np.int32)
        if take:
            written = C.c_uint32(0)
            # a take of no capacity ends a submitted update, whose changes then join, and succeeds only when there is nothing to report
            rc = self._lib.aic_light_changed_take(self._h, int(layer), 0, None, C.byref(written))
            if rc == 0:
                return np.zeros((0, 3), np.int32), bounds
            if rc != 1:  # not AIC_ERR_INVALID
                self._check(rc)
            self._check(self._lib.aic_light_changed_count(self._h, int(layer), C.byref(n), C.c_void_p(bounds.ctypes.data)))
            xyz = np.zeros((max(int(n.value), 1), 3), np.int32)
            self._check(self._lib.aic_light_changed_take(self._h, int(layer), int(n.value), C.c_void_p(xyz.ctypes.data), C.byref(written)))
            return xyz[:written.value], bounds
        self._check(self._lib.aic_light_changed_count(self._h, int(layer), C.byref(n), C.c_void_p(bounds.ctypes.data)))
        return int(n.value), bounds

    @staticmethod
    def _stale_cubes_desc(view_projection, width, height, boxes, light_cubes, expand):
        """(desc, the arrays it points to) of the arguments pick_stale_cubes and probe_stale_cube_rects share"""
        b = np.ascontiguousarray(np.asarray(boxes if boxes is not None else [], np.int32).reshape(-1, 6))
        q = np.ascontiguousarray(np.asarray(light_cubes if light_cubes is not None else [], np.int32).reshape(-1, 3))
        d = StaleCubesDesc()
        d.width, d.height, d.n_boxes, d.n_light_cubes, d.expand = int(width), int(height), len(b), len(q), int(expand)
        d.view_projection = (C.c_double * 16)(*np.asarray(view_projection, np.float64).reshape(16))
        d.boxes = b.ctypes.data if len(b) else None
        d.light_cubes = q.ctypes.data if len(q) else None
        return d, (b, q)

    def pick_stale_cubes(self, view_projection, width: int, height: int, n: int, boxes, light_cubes, src_ptr: int, order_ptr: int, out_ptr: int,
                         cursor: int = 0, max_stale: int = 0, skip_stale: int = 0, flags: int = 0, expand: int = 1) -> StaleCubesInfo:
        """pick_stale from the changed cubes themselves, any number of them (aic_pick_stale_cubes): `boxes` [n, 6] int32 are changed blocks, grown by
        `expand` as under stale_rects(); `light_cubes` [n, 3] int32 are cubes whose light texel changed (Context.light_changed), each the box [q, q + 1)
        grown by one. The device projects them under `view_projection` and marks their rectangles. STALE_DEPTH_TEST is pick_stale's front test;
        STALE_DEPTH_BEHIND lets a light cube's rectangle keep out a world pixel whose depth lies beyond the cube's greatest depth -- exact under
        translucency and antialiasing. The info adds n_rects (rectangles that hold a pixel) and whole_frame."""
        d, keep = self._stale_cubes_desc(view_projection, width, height, boxes, light_cubes, expand)
        d.n, d.max_stale, d.skip_stale, d.cursor, d.flags = int(n), int(max_stale), int(skip_stale), int(cursor), int(flags)
        info = StaleCubesInfo()
        self._check(self._lib.aic_pick_stale_cubes(self._h, C.byref(d), C.c_void_p(src_ptr or None), C.c_void_p(order_ptr or None),
                                                   C.c_void_p(out_ptr or None), C.byref(info)))
        del keep
        return info

    def find_block_cubes(self, layer: int, indices, capacity: int):
        """The cubes of `layer` that hold one of the block `indices`, as runs along z (aic_find_block_cubes): (boxes [n_written, 6] int32 {lo, hi
        exclusive} sorted by a run's first cube in the grid's linear order, info). With more runs than `capacity` the one box info.bounds is written
        instead (none with capacity 0) and info.merged is 1. What a re-evaluated block (replace_blocks) made stale: the grid does not change under
        such a call, only what these cubes look like."""
        idx = np.ascontiguousarray(np.asarray(indices, np.uint32).reshape(-1))
        out = np.zeros((max(int(capacity), 1), 6), np.int32)
        info = BlockCubesInfo()
        self._check(self._lib.aic_find_block_cubes(self._h, int(layer), len(idx), C.c_void_p(idx.ctypes.data if len(idx) else None), int(capacity),
                                                   C.c_void_p(out.ctypes.data if capacity else None), C.byref(info)))
        return out[:info.n_written].copy(), info

    def pick_stale_blocks(self, view_projection, width: int, height: int, n: int, boxes, light_cubes, layer: int, blocks, src_ptr: int, order_ptr: int,
                          out_ptr: int, cursor: int = 0, max_stale: int = 0, skip_stale: int = 0, flags: int = 0, expand: int = 1,
                          max_runs: int = 65536) -> StaleBlocksInfo:
        """pick_stale_cubes with, behind `boxes`, the boxes find_block_cubes(layer, blocks, max_runs) gives, found and kept on the device
        (aic_pick_stale_blocks): the pixels a re-evaluated block made stale first. info.pick is pick_stale_cubes' info, info.found the find's; with
        n = 0 or max_stale = 0 no find runs."""
        d = StaleBlocksDesc()
        d.cubes, keep = self._stale_cubes_desc(view_projection, width, height, boxes, light_cubes, expand)
        d.cubes.n, d.cubes.max_stale, d.cubes.skip_stale, d.cubes.cursor, d.cubes.flags = int(n), int(max_stale), int(skip_stale), int(cursor), int(flags)
        idx = np.ascontiguousarray(np.asarray(blocks if blocks is not None else [], np.uint32).reshape(-1))
        d.layer, d.n_blocks, d.max_runs = int(layer), len(idx), int(max_runs)
        d.block_indices = idx.ctypes.data if len(idx) else None
        info = StaleBlocksInfo()
        self._check(self._lib.aic_pick_stale_blocks(self._h, C.byref(d), C.c_void_p(src_ptr or None), C.c_void_p(order_ptr or None),
                                                    C.c_void_p(out_ptr or None), C.byref(info)))
        del keep, idx
        return info

    def probe_stale_cube_rects(self, view_projection, width: int, height: int, boxes, light_cubes, expand: int = 1) -> np.ndarray:
        """The rectangles pick_stale_cubes projects on the device (aic_probe_stale_cube_rects): [n_boxes + n_light_cubes] STALE_CUBE_RECT_DTYPE records,
        the boxes' first, all zero for a dropped one."""
        d, keep = self._stale_cubes_desc(view_projection, width, height, boxes, light_cubes, expand)
        out = np.zeros(d.n_boxes + d.n_light_cubes, STALE_CUBE_RECT_DTYPE)
        self._check(self._lib.aic_probe_stale_cube_rects(self._h, C.byref(d), C.c_void_p(out.ctypes.data if len(out) else None)))
        del keep
        return out

    def present_split(self, src_ptr: int, src_size, out_size, bloom_intensity: float, tone_mapping: int, maximum_intensity: float, flags: int = 0,
                      out_device: int | None = None):
        """A resident Split frame shown in a window (aic_present_split): stretched with a linear ClampToEdge filter from `src_size` = (width, height) to
        `out_size`, bloomed when `bloom_intensity` > 0, tone-mapped, and encoded as sRGB RGBA8 or, with PRESENT_OUT_F16, as four linear f16 with alpha
        1.0. `src_ptr` is the whole frame in HBM on the context's device; only its colour plane's three colour halves are used. Returns (image, info):
        the image is [height][width][4] uint8 (or uint16: f16 bit patterns) read back to the host, or None when `out_device` -- a device pointer the
        image is written to instead -- is given. Returns once the image is written."""
        d = PresentDesc()
        d.src_width, d.src_height = int(src_size[0]), int(src_size[1])
        d.out_width, d.out_height = int(out_size[0]), int(out_size[1])
        d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = float(bloom_intensity), int(tone_mapping), float(maximum_intensity), int(flags)
        info = PresentInfo()
        if out_device is not None:
            self._check(self._lib.aic_present_split(self._h, C.byref(d), C.c_void_p(src_ptr or None), C.c_void_p(out_device or None), 1, C.byref(info)))
            return None, info
        image = np.zeros((d.out_height, d.out_width, 4), np.uint16 if flags & PRESENT_OUT_F16 else np.uint8)
        self._check(self._lib.aic_present_split(self._h, C.byref(d), C.c_void_p(src_ptr or None), image.ctypes.data_as(C.c_void_p), 0, C.byref(info)))
        return image, info

    def image_cells(self, image, aux, cols: int, rows: int, characters: int, colors: int, exposure: float = 1.0, tone_mapping: int = 0,
                    maximum_intensity: float = float("inf"), postprocessed: bool = False, f16: bool = False, image_device: bool = False,
                    out_device: Optional[int] = None):
        """image_patch_to_character for every cell of an image (aic_image_cells). image: [height][width][4] float32 (or, f16, float16 / uint16 bit
        patterns) of cells_geometry's framebuffer and aux: [height][width] of PIXEL_AUX_DTYPE or None -- or, image_device, two device pointers
        (aux 0: none). Returns (cells [rows][cols] of CELL_DTYPE, info), cells None when `out_device`, a device pointer they are written to, is given."""
        d = CellsDesc(int(cols), int(rows), int(characters), int(colors), float(exposure), int(tone_mapping), float(maximum_intensity), 0)
        d.flags = (CELLS_POSTPROCESSED if postprocessed else 0) | (CELLS_IMAGE_F16 if f16 else 0) | (CELLS_IMAGE_DEVICE if image_device else 0)
        if image_device:
            img_p, aux_p = C.c_void_p(int(image) or None), C.c_void_p(int(aux or 0) or None)
        else:
            image = np.ascontiguousarray(image, (image.dtype if f16 else np.float32))
            if f16 and image.dtype.itemsize != 2:
                raise ValueError("an f16 image is float16 or uint16 bit patterns")
            aux = None if aux is None else np.ascontiguousarray(aux, PIXEL_AUX_DTYPE)
            img_p, aux_p = _ptr(image), (None if aux is None else _ptr(aux))
        info = CellsInfo()
        if out_device is not None:
            d.flags |= CELLS_OUT_DEVICE
            self._check(self._lib.aic_image_cells(self._h, C.byref(d), img_p, aux_p, C.c_void_p(out_device or None), C.byref(info)))
            return None, info
        out = np.zeros((max(int(rows), 1), max(int(cols), 1)), CELL_DTYPE)
        self._check(self._lib.aic_image_cells(self._h, C.byref(d), img_p, aux_p, _ptr(out), C.byref(info)))
        return out, info

    def render_cells(self, frame: FrameDesc, cols: int, rows: int, characters: int, colors: int, out_device: Optional[int] = None):
        """One frame of the terminal renderer (aic_render_cells): `frame`, of cells_geometry's size, is traced into context scratch and turned into
        cells on the device. Returns (cells [rows][cols] of CELL_DTYPE or None with `out_device`, frame info, cells info)."""
        d = CellsDesc(int(cols), int(rows), int(characters), int(colors), 1.0, 0, float("inf"), 0)
        fi, ci = FrameInfo(), CellsInfo()
        if out_device is not None:
            self._check(self._lib.aic_render_cells(self._h, C.byref(frame), C.byref(d), C.c_void_p(out_device or None), 1, C.byref(fi), C.byref(ci)))
            return None, fi, ci
        out = np.zeros((max(int(rows), 1), max(int(cols), 1)), CELL_DTYPE)
        self._check(self._lib.aic_render_cells(self._h, C.byref(frame), C.byref(d), _ptr(out), 0, C.byref(fi), C.byref(ci)))
        return out, fi, ci

    def export_split(self, src, src_size, out_size, inverse_projection_zw, color: bool = True, depth: bool = True, device_outs=None):
        """A resident Split frame exported as sRGB8 colour and metric depth (aic_export_split): the colour is what present_split gives at `out_size`
        without bloom or tone mapping; the depth is the nearest depth texel as a distance along the view axis, 0 where there is no surface (a UI pixel,
        the sky, a marker of an unfilled reprojection). `src` is the whole frame of `src_size` = (width, height) in HBM on the context's device;
        `inverse_projection_zw` = {ipz.z, ipw.z, ipz.w, ipw.w} of the camera's inverse projection, as reproject_split takes it. Returns (colour, depth,
        info): [height][width][4] uint8 and [height][width] float32 read back to the host, None for a plane not asked for. With `device_outs` = (colour
        pointer, depth pointer) -- either may be 0 or None -- the planes are written to that device memory instead and both returned planes are None.
        info.n_surface, depth_min and depth_max cover the pixels with a finite depth > 0, whatever planes are asked for."""
        d = ExportDesc()
        d.src_width, d.src_height = int(src_size[0]), int(src_size[1])
        d.out_width, d.out_height = int(out_size[0]), int(out_size[1])
        d.inverse_projection_zw[:] = [float(v) for v in np.asarray(inverse_projection_zw, np.float32).reshape(4)]
        info = ExportInfo()
        if device_outs is not None:
            self._check(self._lib.aic_export_split(self._h, C.byref(d), C.c_void_p(src or None), C.c_void_p(device_outs[0] or None), C.c_void_p(device_outs[1] or None), 1,
                                                   C.byref(info)))
            return None, None, info
        rgba = np.zeros((d.out_height, d.out_width, 4), np.uint8) if color else None
        dist = np.zeros((d.out_height, d.out_width), np.float32) if depth else None
        self._check(self._lib.aic_export_split(self._h, C.byref(d), C.c_void_p(src or None), rgba.ctypes.data_as(C.c_void_p) if color else None,
                                               dist.ctypes.data_as(C.c_void_p) if depth else None, 0, C.byref(info)))
        return rgba, dist, info

    def present_split_lines(self, src_ptr: int, src_size, out_size, bloom_intensity: float, tone_mapping: int, maximum_intensity: float, view_projection,
                            vertices=None, n_lines: int | None = None, flags: int = 0, out_device: int | None = None):
        """present_split with a line list drawn into the scene before bloom and tone mapping, depth-tested against the frame's depth plane
        (aic_present_split_lines). `view_projection` = [16] column-major projection x view; `vertices` = [2 n] line vertices on the host (anything
        np.asarray turns into n x 2 x 7 float32: LINE_VERTEX_DTYPE records, or position + linear RGBA rows), or a device pointer (an int) with
        `n_lines`; None: no lines. Returns (image or None, info, lines_info) as present_split does."""
        d = PresentDesc()
        d.src_width, d.src_height = int(src_size[0]), int(src_size[1])
        d.out_width, d.out_height = int(out_size[0]), int(out_size[1])
        d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = float(bloom_intensity), int(tone_mapping), float(maximum_intensity), int(flags)
        ld = LinesDesc()
        ld.view_projection[:] = [float(v) for v in np.asarray(view_projection, np.float32).reshape(16)]
        keep = None
        if isinstance(vertices, int):
            ld.vertices, ld.n_lines, ld.flags = vertices, int(n_lines), LINES_DEVICE
        elif vertices is not None:
            keep = np.asarray(vertices)
            keep = np.ascontiguousarray(keep.view(np.float32) if keep.dtype == LINE_VERTEX_DTYPE else keep, np.float32).reshape(-1, 2, 7)
            ld.vertices, ld.n_lines = keep.ctypes.data, len(keep) if n_lines is None else int(n_lines)
        info, lines_info = PresentInfo(), LinesInfo()
        if out_device is not None:
            self._check(self._lib.aic_present_split_lines(self._h, C.byref(d), C.byref(ld), C.c_void_p(src_ptr or None), C.c_void_p(out_device or None), 1,
                                                          C.byref(info), C.byref(lines_info)))
            return None, info, lines_info
        image = np.zeros((d.out_height, d.out_width, 4), np.uint16 if flags & PRESENT_OUT_F16 else np.uint8)
        self._check(self._lib.aic_present_split_lines(self._h, C.byref(d), C.byref(ld), C.c_void_p(src_ptr or None), image.ctypes.data_as(C.c_void_p), 0,
                                                      C.byref(info), C.byref(lines_info)))
        return image, info, lines_info

    def set_text_font(self, atlas, cell_width: int = 0, cell_height: int = 0, cell_margin: int = 0) -> None:
        """The font atlas of the info text (aic_set_text_font): `atlas` = [16 * cell_height][16 * cell_width][4] uint8, premultiplied RGBA8, the cell of
        code k at column k % 16, row k / 16, with `cell_margin` texels on every side outside the logical cell; None drops the font. Copied to the
        device, resident until replaced."""
        if atlas is None:
            self._check(self._lib.aic_set_text_font(self._h, None, 0, 0, 0))
            return
        keep = np.ascontiguousarray(atlas, np.uint8)
        if keep.shape != (16 * int(cell_height), 16 * int(cell_width), 4):
            raise ValueError(f"set_text_font: atlas of shape {keep.shape} for cells of {cell_width} x {cell_height}")
        self._check(self._lib.aic_set_text_font(self._h, keep.ctypes.data_as(C.c_void_p), int(cell_width), int(cell_height), int(cell_margin)))

    def present_split_text(self, src_ptr: int, src_size, out_size, bloom_intensity: float, tone_mapping: int, maximum_intensity: float, text=None,
                           view_projection=None, vertices=None, n_lines: int | None = None, flags: int = 0, out_device: int | None = None):
        """present_split_lines with the info text laid over the tone-mapped scene (aic_present_split_text). `text` = (codes, scale, origin): codes a
        [rows][cols] uint8 array on the host, or (device pointer, cols, rows); scale and origin as text_geometry gives them; None: no text. Lines as in
        present_split_lines, with view_projection None for none. Returns (image or None, info, lines_info)."""
        d = PresentDesc()
        d.src_width, d.src_height = int(src_size[0]), int(src_size[1])
        d.out_width, d.out_height = int(out_size[0]), int(out_size[1])
        d.bloom_intensity, d.tone_mapping, d.maximum_intensity, d.flags = float(bloom_intensity), int(tone_mapping), float(maximum_intensity), int(flags)
        ld, keep = None, None
        if view_projection is not None:
            ld = LinesDesc()
            ld.view_projection[:] = [float(v) for v in np.asarray(view_projection, np.float32).reshape(16)]
            if isinstance(vertices, int):
                ld.vertices, ld.n_lines, ld.flags = vertices, int(n_lines), LINES_DEVICE
            elif vertices is not None:
                keep = np.asarray(vertices)
                keep = np.ascontiguousarray(keep.view(np.float32) if keep.dtype == LINE_VERTEX_DTYPE else keep, np.float32).reshape(-1, 2, 7)
                ld.vertices, ld.n_lines = keep.ctypes.data, len(keep) if n_lines is None else int(n_lines)
        td, keep_codes = None, None
        if text is not None:
            codes, scale, origin = text
            td = TextDesc()
            td.scale[:], td.origin[:] = [float(v) for v in scale], [float(v) for v in origin]
            if isinstance(codes, tuple):
                td.codes, td.cols, td.rows, td.flags = codes[0], int(codes[1]), int(codes[2]), TEXT_DEVICE
            else:
                keep_codes = np.ascontiguousarray(codes, np.uint8)
                td.codes, td.rows, td.cols = keep_codes.ctypes.data, keep_codes.shape[0], keep_codes.shape[1]
        info, lines_info = PresentInfo(), LinesInfo()
        args = (C.byref(d), C.byref(ld) if ld is not None else None, C.byref(td) if td is not None else None, C.c_void_p(src_ptr or None))
        if out_device is not None:
            self._check(self._lib.aic_present_split_text(self._h, *args, C.c_void_p(out_device or None), 1, C.byref(info), C.byref(lines_info)))
            return None, info, lines_info
        image = np.zeros((d.out_height, d.out_width, 4), np.uint16 if flags & PRESENT_OUT_F16 else np.uint8)
        self._check(self._lib.aic_present_split_text(self._h, *args, image.ctypes.data_as(C.c_void_p), 0, C.byref(info), C.byref(lines_info)))
        return image, info, lines_info

    def render_submit(self, frame: FrameDesc, device_ptr: int, slot: int) -> None:
        """Queues a frame on `slot` (0..MAX_IN_FLIGHT-1); returns without waiting (aic_render_submit). A FRAME_OUT_SPLIT frame leaves 12 bytes per
        pixel at `device_ptr`: `split_planes` views a host copy of them as the two planes."""
        self._check(self._lib.aic_render_submit(self._h, C.byref(frame), C.c_void_p(device_ptr), int(slot)))

    def render_submit_batch(self, frames, device_ptrs, slot: int) -> None:
        """aic_render_submit_batch: 1, 2, 4 or 8 frames (same size, partition, flags) traced by one launch, frame i into device_ptrs[i]."""
        arr = (FrameDesc * len(frames))(*frames)
        ptrs = (C.c_void_p * len(frames))(*[int(p) for p in device_ptrs])
        self._check(self._lib.aic_render_submit_batch(self._h, len(frames), arr, ptrs, slot))

    def render_wait_batch(self, slot: int, n_frames: int):
        infos = (FrameInfo * n_frames)()
        self._check(self._lib.aic_render_wait_batch(self._h, slot, n_frames, infos))
        return list(infos)

    def render_wait(self, slot: int) -> FrameInfo:
        info = FrameInfo()
        self._check(self._lib.aic_render_wait(self._h, int(slot), C.byref(info)))
        return info

    def assemble_strips(self, gathered_ptr: int, out_ptr: int, width: int, height: int, strip_rows: int, n_parts: int) -> None:
        self._check(self._lib.aic_assemble_strips(self._h, C.c_void_p(gathered_ptr), C.c_void_p(out_ptr), width, height, strip_rows, n_parts))

    def synchronize(self) -> None:
        self._check(self._lib.aic_synchronize(self._h))

    def stream_wait_frame(self, slot: int, hip_stream: int) -> None:
        """`hip_stream` (a raw hipStream_t, e.g. torch.cuda.current_stream().cuda_stream) waits on the device for the frame
        submitted on `slot`; the host does not block (aic_stream_wait_frame)."""
        self._check(self._lib.aic_stream_wait_frame(self._h, int(slot), C.c_void_p(hip_stream)))

    def wait_event(self, hip_event: int) -> None:
        """Everything the context queues from now on waits for the caller's hipEvent_t (aic_wait_event)."""
        self._check(self._lib.aic_wait_event(self._h, C.c_void_p(hip_event)))

    # -- probes ----------------------------------------------------------------------------
    def probe_raycast(self, origin, direction, bounds=None, include_exit=True, max_steps=64):
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        d = np.ascontiguousarray(direction, np.float64).reshape(3)
        lo = np.zeros(3, np.int32) if bounds is None else np.ascontiguousarray(bounds[0], np.int32)
        hi = np.zeros(3, np.int32) if bounds is None else np.ascontiguousarray(bounds[1], np.int32)
        out = np.zeros(max_steps, RC_STEP_DTYPE)
        n = C.c_uint32(0)
        ended = C.c_int(0)
        self._check(self._lib.aic_probe_raycast(self._h, o.ctypes.data, d.ctypes.data, int(bounds is not None), lo.ctypes.data,
                                                hi.ctypes.data, int(include_exit), max_steps, out.ctypes.data, C.byref(n), C.byref(ended)))
        return out[: n.value], bool(ended.value)

    def probe_powf(self, x, y) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        out = np.zeros(x.shape, np.float32)
        self._check(self._lib.aic_probe_powf(self._h, _ptr(x), _ptr(y), x.size, _ptr(out)))
        return out

    def probe_expf(self, x) -> np.ndarray:
        """The device's expf (distance_fog's f32::exp) of every element of `x` (|x| < 88)."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(x.shape, np.float32)
        self._check(self._lib.aic_probe_expf(self._h, _ptr(x), x.size, _ptr(out)))
        return out

    def probe_bloom(self, colorbuf, exposure: float, options: "Options", want_mip0: bool = False):
        """AIC_FRAME_BLOOM's post-process on a ColorBuf ([h][w][4] float32: l0, l1, l2, t) with `options`' bloom_intensity (even 0), tone mapping and
        maximum intensity: returns the RGBA8 frame [h][w][4], and with want_mip0 also the chain's mip 0 as float16 [T0y][T0x][4]."""
        cb = np.ascontiguousarray(colorbuf, np.float32)
        if cb.ndim != 3 or cb.shape[2] != 4:
            raise ValueError("colorbuf must be [h][w][4]")
        h, w = cb.shape[:2]
        out = np.zeros((h, w, 4), np.uint8)
        size = (C.c_uint32 * 2)()
        t0 = bloom_geometry(w, h)[1]
        mip0 = np.zeros((t0[1], t0[0], 4), np.float16) if want_mip0 else None
        self._check(self._lib.aic_probe_bloom(self._h, w, h, _ptr(cb), float(exposure), C.byref(options), _ptr(out),
                                              _ptr(mip0) if mip0 is not None else None, C.byref(size)))
        assert (size[0], size[1]) == t0, ((size[0], size[1]), t0)
        return (out, mip0) if want_mip0 else out

    def evaluate_light(self, layer: int, maximum_distance: int, fast: bool = True, epsilon: int = 1, batch: int = 32,
                       queue_order: int = 16, queue=None, max_updates: int = 0, lanes_per_cube: int = 0, session: bool = False,
                       dep_pool_chunks: int = 0) -> LightInfo:
        """`Mutation::fast_evaluate_light` (if `fast`) then `Mutation::evaluate_light(epsilon)` (space.rs:1496-1540) on
        the uploaded space, compute_light on the device. `queue`: None = every Uninitialized texel (when not `fast`), or a
        list of ((x, y, z), priority). The layer's light volume is updated in place."""
        hooks = (LIGHT_HOOK_SESSION if session else 0) | ((int(dep_pool_chunks) & 0xffff) << LIGHT_HOOK_POOL_SHIFT)  # (test hooks: aic_light_params.hooks)
        p = LightParams(maximum_distance, int(fast), epsilon, batch, queue_order, -1, lanes_per_cube, hooks, None, None, max_updates)
        keep = []
        if queue is not None:
            qc = np.ascontiguousarray([q[0] for q in queue], np.int32).reshape(-1, 3)
            qp = np.ascontiguousarray([q[1] for q in queue], np.int32)
            keep = [qc, qp]
            p.n_queue = len(qp)
            p.queue_cubes = qc.ctypes.data
            p.queue_priorities = qp.ctypes.data
        info = LightInfo()
        self._check(self._lib.aic_evaluate_light(self._h, layer, C.byref(p), C.byref(info)))
        del keep
        return info

    def evaluate_light_submit(self, layer: int, maximum_distance: int, fast: bool = True, epsilon: int = 1, batch: int = 32, queue_order: int = 16,
                              queue=None, max_updates: int = 0, lanes_per_cube: int = 0) -> None:
        """aic_evaluate_light_submit: the same update on the context's worker thread; `evaluate_light_wait` publishes and reports it."""
        p = LightParams(maximum_distance, int(fast), epsilon, batch, queue_order, -1, lanes_per_cube, 0, None, None, max_updates)
        keep = []
        if queue is not None:
            qc = np.ascontiguousarray([q[0] for q in queue], np.int32).reshape(-1, 3)
            qp = np.ascontiguousarray([q[1] for q in queue], np.int32)
            keep = [qc, qp]
            p.n_queue = len(qp)
            p.queue_cubes = qc.ctypes.data
            p.queue_priorities = qp.ctypes.data
        self._check(self._lib.aic_evaluate_light_submit(self._h, layer, C.byref(p)))
        del keep  # (the library copied the arrays)

    def evaluate_light_done(self, layer: int) -> bool:
        """aic_evaluate_light_poll: False while a submitted update is still running."""
        d = C.c_int(1)
        self._check(self._lib.aic_evaluate_light_poll(self._h, layer, C.byref(d)))
        return bool(d.value)

    def evaluate_light_wait(self, layer: int) -> LightInfo:
        info = LightInfo()
        self._check(self._lib.aic_evaluate_light_wait(self._h, layer, C.byref(info)))
        return info

    def light_cubes_changed(self, layer: int, xyz, queue_order: int = 16) -> None:
        """`modified_cube_needs_update` (updater.rs:135-173) for cubes just changed with `update_cubes`: queues them and their
        neighbours on the layer's light update queue (drained by `evaluate_light(fast=False, queue=[])`)."""
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        self._check(self._lib.aic_light_cubes_changed(self._h, layer, len(xyz), _ptr(xyz), queue_order))

    def read_light_volume(self, layer: int, shape) -> np.ndarray:
        out = np.zeros(tuple(shape) + (4,), np.uint8)
        self._check(self._lib.aic_read_light_volume(self._h, layer, out.ctypes.data))
        return out

    def read_light_cubes(self, layer: int, xyz) -> np.ndarray:
        """The texels of the listed cubes, [n][4] (`LightStorage::get`, light/data.rs, over a list)."""
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        out = np.zeros((len(xyz), 4), np.uint8)
        self._check(self._lib.aic_read_light_cubes(self._h, layer, len(xyz), _ptr(xyz), out.ctypes.data))
        return out

    def probe_derived(self, layer: int, n_blocks: int):
        out = np.zeros((n_blocks, 32), np.float32)
        opq = np.zeros((n_blocks, 6), np.uint8)
        self._check(self._lib.aic_probe_derived(self._h, layer, out.ctypes.data, opq.ctypes.data))
        return out, opq

    def probe_cube_grid(self, layer: int, shape, n_blocks: int):
        """The layer's cube grid as it stands on the device (test hook): (grid u16 [sx, sy, sz] -- indices with their tags where the
        grid carries them, csrc/aic_device.h --, class table u32 [ceil(n_blocks / 16)], 2 bits per block index, whether the grid is tagged)."""
        grid = np.zeros(tuple(int(v) for v in shape), np.uint16)
        cls = np.zeros((int(n_blocks) + 15) // 16, np.uint32)
        tagged = C.c_uint32(0)
        # (an array of no elements still has an address: the library rejects NULL, and writes nothing there)
        self._check(self._lib.aic_probe_cube_grid(self._h, layer, grid.ctypes.data, _ptr(cls), C.byref(tagged)))
        return grid, cls, bool(tagged.value)

    def probe_log2f(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(x.shape, np.float32)
        self._check(self._lib.aic_probe_log2f(self._h, _ptr(x), x.size, _ptr(out)))
        return out

    def probe_light_lut(self) -> np.ndarray:
        out = np.zeros(256, np.float32)
        self._check(self._lib.aic_probe_light_lut(self._h, out.ctypes.data))
        return out


class MultiContext:
    """`aic_multi`: one object over several devices (ids may repeat), the form a Rust `HipRtRenderer` would hold.
    Scene calls are replicated; `render` deals 8-row strips to the devices and assembles the frame on the first."""

    def __init__(self, device_ids):
        self._lib = load()
        lib = self._lib
        lib.aic_create_multi.restype = C.c_void_p
        lib.aic_create_multi.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        lib.aic_destroy_multi.argtypes = [C.c_void_p]
        lib.aic_multi_last_error.restype = C.c_char_p
        lib.aic_multi_last_error.argtypes = [C.c_void_p]
        lib.aic_multi_device_count.argtypes = [C.c_void_p]
        lib.aic_multi_upload_space.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_multi_clear_space.argtypes = [C.c_void_p, C.c_int]
        lib.aic_multi_set_options.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_multi_set_depth_transform.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        lib.aic_multi_update_light_volume.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_multi_evaluate_light.argtypes = [C.c_void_p, C.c_int, C.POINTER(LightParams), C.POINTER(LightInfo)]
        lib.aic_multi_light_cubes_changed.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_int]
        lib.aic_multi_update_cubes.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.aic_multi_render.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.aic_multi_render_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
        lib.aic_multi_render_wait.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        ids = np.ascontiguousarray(device_ids, np.int32)
        st = C.c_int(0)
        self._h = lib.aic_create_multi(len(ids), _ptr(ids), C.byref(st))
        if not self._h:
            raise AicError(st.value, "aic_create_multi failed (no usable MI355X?)")

    def close(self) -> None:
        if self._h:
            self._lib.aic_destroy_multi(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != AIC_OK:
            raise AicError(rc, self._lib.aic_multi_last_error(self._h).decode())

    @property
    def device_count(self) -> int:
        return int(self._lib.aic_multi_device_count(self._h))

    def upload_space(self, layer: int, flat_space) -> None:
        d, _keep = Context._space_desc(flat_space)
        self._check(self._lib.aic_multi_upload_space(self._h, layer, C.byref(d)))

    def clear_space(self, layer: int) -> None:
        self._check(self._lib.aic_multi_clear_space(self._h, layer))

    def set_options(self, layer: int, options: Options) -> None:
        self._check(self._lib.aic_multi_set_options(self._h, layer, C.byref(options)))

    def set_depth_transform(self, zw) -> None:
        self._check(self._lib.aic_multi_set_depth_transform(self._h, (C.c_double * 4)(*[float(v) for v in zw])))

    def update_light_volume(self, layer: int, light) -> None:
        lt = np.ascontiguousarray(light, np.uint8)
        self._check(self._lib.aic_multi_update_light_volume(self._h, layer, _ptr(lt)))

    def evaluate_light(self, layer: int, maximum_distance: int, fast: bool = True, epsilon: int = 1, batch: int = 32, queue_order: int = 16) -> LightInfo:
        p = LightParams(maximum_distance, int(fast), epsilon, batch, queue_order, -1, 0, 0, None, None, 0)
        info = LightInfo()
        self._check(self._lib.aic_multi_evaluate_light(self._h, layer, C.byref(p), C.byref(info)))
        return info

    def light_cubes_changed(self, layer: int, xyz, queue_order: int = 16) -> None:
        """`Context.light_cubes_changed` on the device that runs the updater; the texels it writes reach the others at once."""
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        self._check(self._lib.aic_multi_light_cubes_changed(self._h, layer, len(xyz), _ptr(xyz), queue_order))

    def update_cubes(self, layer: int, xyz, block_index=None, light=None) -> None:
        xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
        bi = None if block_index is None else np.ascontiguousarray(block_index, np.uint16)
        lt = None if light is None else np.ascontiguousarray(light, np.uint8).reshape(-1, 4)
        self._check(self._lib.aic_multi_update_cubes(self._h, layer, len(xyz), _ptr(xyz), _ptr(bi), _ptr(lt)))

    def render(self, frame: FrameDesc):
        out = np.zeros((frame.height, frame.width, 4), np.uint8)
        info = FrameInfo()
        self._check(self._lib.aic_multi_render(self._h, C.byref(frame), _ptr(out), 0, C.byref(info)))
        return {"rgba8": out, "info": info}

    def render_submit(self, frame: FrameDesc, slot: int, device_ptr: int = 0):
        """aic_multi_render_submit: the frame is queued on `slot` of every device; returns the host array the wait fills (or None: device_ptr)."""
        out = None if device_ptr else np.zeros((frame.height, frame.width, 4), np.uint8)
        self._check(self._lib.aic_multi_render_submit(self._h, C.byref(frame), C.c_void_p(device_ptr) if device_ptr else _ptr(out), 1 if device_ptr else 0, slot))
        return out

    def render_wait(self, slot: int) -> FrameInfo:
        info = FrameInfo()
        self._check(self._lib.aic_multi_render_wait(self._h, slot, C.byref(info)))
        return info
