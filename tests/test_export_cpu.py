"""The RGB-D export of a resident Split frame without a GPU (aic_export_split, aic_export_size; DESIGN.md "Export"): the NumPy restatement
tests/export_ref.py against values worked out by hand, the size policy and the pinhole of the host mirror against the reference's formulas
(all-is-cubes-gpu/src/rerun_image.rs:302-338), and the binding's symbols and struct sizes."""
import ctypes as C
import math

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import export_ref as ref

F = np.float32
MARKER = (0, 0, 0, 0xBC00)
IPZW = (0.25, -1.0, 1.0, 0.5)  # -(d / 4 - 1) / (d + 1 / 2)


def h16(*values):
    return np.array(values, np.float16).view(np.uint16)


def frame_2x2(third_depth):
    """One texel for each rule, row-major: a UI pixel (rule 1), a marker over a plain depth (rule 2), `third_depth`, a surface at depth 0.5 (rule 4)."""
    color = np.zeros((2, 2, 4), np.uint16)
    color[0, 0] = h16(1.0, 0.0, 0.0, 1.0)
    color[0, 1] = MARKER
    color[1, 0] = h16(0.0, 1.0, 0.0, 1.0)
    color[1, 1] = h16(2.0, np.inf, 65504.0, 0.25)
    depth = np.array([[-0.5, 0.25], [third_depth, 0.5]], F)
    return color, depth


def test_the_restatement_against_values_by_hand():
    # rule 4 at d = 0.5: -(0.125 - 1) / (0.5 + 0.5) = 0.875, every step exact
    color, depth = frame_2x2(1.0)  # rule 3: the far plane
    rgba, z, stats = ref.export(color, depth, IPZW, (2, 2))
    assert z.dtype == F and z.tolist() == [[0.0, 0.0], [0.0, 0.875]]
    assert stats == (1, F(0.875), F(0.875))
    assert rgba.dtype == np.uint8 and rgba.tolist() == [[[255, 0, 0, 255], [0, 0, 0, 255]], [[0, 255, 0, 255], [255, 255, 255, 255]]]
    # one ulp below the far plane is a surface. d = 1 - 2^-24: d / 4 - 1 = -0.75 - 2^-26 rounds to -0.75 (a quarter ulp); d + 0.5 = 1.5 - 2^-24 is a tie
    # between 1.5 - 2^-23 (odd) and 1.5 (even) and rounds to 1.5; 0.75 / 1.5 = 0.5
    below = np.nextafter(F(1.0), F(0.0))
    color, depth = frame_2x2(below)
    _, z, stats = ref.export(color, depth, IPZW, (2, 2))
    assert z.tolist() == [[0.0, 0.0], [0.5, 0.875]]
    assert stats == (2, F(0.5), F(0.875))
    # -0.0 and NaN are rule 1's; a marker wins over any depth but is asked after the sign
    for none in (F(-0.0), F(np.nan)):
        _, z, _ = ref.export(*frame_2x2(none), IPZW, (2, 2))
        assert z.tolist() == [[0.0, 0.0], [0.0, 0.875]]
    # nearest, never interpolated: at 4 x 4 every texel covers 2 x 2 pixels (u = 1/8, 3/8, 5/8, 7/8 -> texels 0, 0, 1, 1); at 1 x 1 the centre
    # u = v = 1/2 falls on texel min(uint(0.5 * 2), 1) = 1 of either axis
    color, depth = frame_2x2(below)
    _, z, stats = ref.export(color, depth, IPZW, (4, 4))
    assert z.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0.5, 0.5, 0.875, 0.875], [0.5, 0.5, 0.875, 0.875]]
    assert stats == (8, F(0.5), F(0.875))
    _, z, stats = ref.export(color, depth, IPZW, (1, 1))
    assert z.tolist() == [[0.875]] and stats == (1, F(0.875), F(0.875))
    # no surface at all
    color, depth = frame_2x2(1.0)
    depth[1, 1] = 1.0
    assert ref.export(color, depth, IPZW, (3, 2))[2] == (0, F(0.0), F(0.0))
    # a depth that unprojects to something not finite or not positive is exported as it is and not counted: d = 4 gives -(1 - 1) / 4.5 = -0.0
    color, depth = frame_2x2(4.0)
    _, z, stats = ref.export(color, depth, (0.25, -1.0, 1.0, 0.5), (2, 2))
    assert z[1, 0] == 0.0 and np.signbit(z[1, 0]) and stats[0] == 1
    _, z, stats = ref.export(color, depth, (0.25, -1.0, 1.0, -0.5), (2, 2))  # d = 0.5: -(-0.875) / 0 = +inf
    assert np.isposinf(z[1, 1]) and z[1, 0] == 0.0 and stats == (0, F(0.0), F(0.0))  # (d = 4: -0.0 / 3.5; neither is a surface)


def by_formula(w, h, cap):
    area = float(w) * float(h)
    if area <= cap:
        return w, h
    r = math.sqrt(cap / area)
    return math.ceil(w * r), math.ceil(h * r)


@pytest.mark.parametrize("size", [(640, 480), (1920, 1080), (641, 480), (65535, 65535), (0, 7), (7, 0), (1, 1)])
def test_export_size_is_the_reference_policy(size):
    for cap in (640.0 * 480.0, 1.0, 1e12):
        want = by_formula(*size, cap)
        assert abi.export_size(size, cap) == want, (size, cap)
        assert ref.export_size(size, cap) == want, (size, cap)
    assert abi.export_size(size) == by_formula(*size, 640.0 * 480.0)
    assert tuple(H.logged_image_size_policy(size)) == abi.export_size(size)


def test_export_size_values_and_rejections():
    assert abi.export_size((640, 480)) == (640, 480)
    assert abi.export_size((1920, 1080)) == (740, 416)
    assert abi.export_size((641, 480)) == (641, 480)  # r = 0.99922: ceil(640.4999), ceil(479.63) -- rounding up gives the size back
    assert abi.export_size((640, 480), 1.0) == (2, 1)  # r = 1 / 554.26: ceil(1.155), ceil(0.866)
    assert abi.export_size((0, 7), 1.0) == (0, 7)
    lib = abi.load()
    out = (C.c_uint32 * 2)(5, 6)
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        with pytest.raises(abi.AicError):
            abi.export_size((8, 8), bad)
        assert lib.aic_export_size(8, 8, bad, out) == 1 and tuple(out) == (5, 6)
    assert lib.aic_export_size(8, 8, 64.0, None) == 1


@pytest.mark.parametrize("fov_y", [90.0, 60.0, 120.0])
@pytest.mark.parametrize("size", [(640, 480), (416, 740)])
def test_pinhole_is_convert_camera_to_pinhole(fov_y, size):
    o = H.GraphicsOptions()
    o.fov_y = fov_y
    camera = H.Camera(o, H.Viewport.with_scale(1.0, *size))
    camera.look_at_y_up((0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    matrix, resolution, transform = camera.pinhole()
    want = ref.pinhole(fov_y, *size)
    assert matrix.dtype == F and matrix.shape == (9,) and (matrix.view(np.uint32) == want.view(np.uint32)).all(), (matrix, want)
    assert resolution.dtype == F and resolution.tolist() == [float(size[0]), float(size[1])]
    assert transform.rotation == camera.view_transform().rotation and transform.translation == camera.view_transform().translation
    # what the matrix means: the image centre is the principal point, and a point on the edge of the vertical field of view lands on the image's edge
    assert matrix[6] == size[0] / 2 and matrix[7] == size[1] / 2 and matrix[8] == 1.0
    assert matrix[4] * math.tan(math.radians(fov_y / 2)) == pytest.approx(size[1] / 2, rel=1e-6)
    assert matrix[0] == pytest.approx(matrix[4], rel=1e-6)  # square pixels


def test_symbols_and_struct_layouts():
    assert "aic_export_split" in abi.ABI_SYMBOLS and "aic_export_size" in abi.ABI_SYMBOLS
    lib = abi.load()
    assert len(lib.aic_export_split.argtypes) == 7 and lib.aic_export_split.argtypes[0] is C.c_void_p
    assert len(lib.aic_export_size.argtypes) == 4 and lib.aic_export_size.argtypes[2] is C.c_double
    assert C.sizeof(abi.ExportDesc) == 48
    assert C.sizeof(abi.ExportInfo) == 32
    assert [name for name, _ in abi.ExportDesc._fields_] == ["src_width", "src_height", "out_width", "out_height", "inverse_projection_zw", "flags", "reserved"]
    assert [name for name, _ in abi.ExportInfo._fields_] == ["kernel_ms", "n_surface", "depth_min", "depth_max", "reserved"]
    assert callable(abi.Context.export_split)
