"""NumPy restatement of the RGB-D export of a resident Split frame (aic_export_split; DESIGN.md "Export"), for the tests.

Colour: the presentation's scene texel at the logged size (tests/present_ref.py's `scene`) through the project's sRGB8 encoder (tests/bloom_ref.py's
`encode`), alpha byte 255 -- aic_present_split without bloom or tone mapping. Depth: the nearest depth texel, never interpolated
(all-is-cubes-gpu shaders/rerun-copy.wgsl:73-88), as a distance along the view axis by the reprojection's linearisation (tests/reproject_ref.py's `_lin`),
0 where there is no surface. Every step is float32 in the order DESIGN.md writes it.
"""
from __future__ import annotations

import numpy as np

from tests import bloom_ref, present_ref, reproject_ref

F = np.float32


def color(color_bits, out_w: int, out_h: int):
    """[out_h][out_w][4] uint8 from the frame's colour plane [h][w][4] uint16."""
    s = present_ref.scene(color_bits, out_w, out_h)
    return bloom_ref.encode(s[..., :3], np.ones(s.shape[:2], F))


def nearest(src_w: int, src_h: int, out_w: int, out_h: int):
    """(iy [out_h][out_w], ix [out_h][out_w]): the source texel of every output pixel. u = (x + 0.5) / out_w in float32, ix = min(uint(u * src_w), src_w - 1)."""
    u, v = bloom_ref._centres(out_w, out_h)
    ix = np.minimum((u * F(src_w)).astype(np.int64), src_w - 1)
    iy = np.minimum((v * F(src_h)).astype(np.int64), src_h - 1)
    return iy, ix


def depth(color_bits, depth_plane, ipzw, out_w: int, out_h: int):
    """[out_h][out_w] float32 from the frame's two planes (depth_plane: float32, or uint32 bit patterns). In this order: 0 for a texel with its sign bit
    set or a NaN; 0 where the colour texel is the marker (alpha not above -0.5); 0 for 1.0; else -(d a + b) / (d c + e)."""
    color_bits = np.ascontiguousarray(color_bits, np.uint16)
    bits = np.ascontiguousarray(depth_plane).view(np.uint32)
    h, w = bits.shape
    iy, ix = nearest(w, h, out_w, out_h)
    d_bits = bits[iy, ix]
    d = d_bits.view(F)
    c = color_bits[iy, ix]
    none = ((d_bits >> 31) != 0) | np.isnan(d) | ~reproject_ref.valid(c) | (d == F(1.0))
    with np.errstate(all="ignore"):
        z = reproject_ref._lin(np.where(none, F(0.0), d), np.asarray(ipzw, F))
    return np.where(none, F(0.0), z).astype(F)


def statistics(z):
    """(n_surface, depth_min, depth_max) over the pixels whose exported depth is finite and > 0; (0, 0, 0) when there are none."""
    z = np.asarray(z, F)
    with np.errstate(invalid="ignore"):
        surface = np.isfinite(z) & (z > 0)
    if not surface.any():
        return 0, F(0.0), F(0.0)
    return int(surface.sum()), z[surface].min(), z[surface].max()


def export(color_bits, depth_plane, ipzw, out_size):
    """aic_export_split into out_size = (width, height): (colour uint8 [h][w][4], depth float32 [h][w], (n_surface, depth_min, depth_max))."""
    z = depth(color_bits, depth_plane, ipzw, *out_size)
    return color(color_bits, *out_size), z, statistics(z)


def export_size(size, max_area=640.0 * 480.0):
    """logged_image_size_policy (rerun_image.rs:302-311) in float64, the cap a parameter."""
    w, h = int(size[0]), int(size[1])
    area = float(w) * float(h)
    if area <= max_area:
        return w, h
    r = np.sqrt(np.float64(max_area) / np.float64(area))
    return int(np.ceil(np.float64(w) * r)), int(np.ceil(np.float64(h) * r))


def pinhole(fov_y_degrees: float, width: int, height: int):
    """convert_camera_to_pinhole (rerun_image.rs:314-338): the column-major 3 x 3 in float32. The tangent is taken in float64 and then rounded."""
    import math

    w, h = F(width), F(height)
    half_w, half_h = w * F(0.5), h * F(0.5)
    aspect = w / h
    tan_y = F(math.tan((float(fov_y_degrees) * 0.5) * (math.pi / 180.0)))
    tan_x = tan_y * aspect
    return np.array([half_w / tan_x, 0, 0, 0, half_h / tan_y, 0, half_w, half_h, 1], F)
