"""AIC_FRAME_OUT_SPLIT without a device: the header, the ctypes binding and the Rust shim agree on the new constant and entry points, and the host
mirror's Camera::depth_transform_zw is raytrace_to_texture's depth transform (raytrace_to_texture.rs:613-618) bit for bit."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "aic_hip.h").read_text()
FFI = (ROOT / "rust" / "all-is-cubes-hip" / "src" / "ffi.rs").read_text()
SHIM = (ROOT / "rust" / "all-is-cubes-hip" / "src" / "lib.rs").read_text()


def test_constant_agrees_everywhere():
    m = re.search(r"#define AIC_FRAME_OUT_SPLIT (\d+)u", HEADER)
    assert m and int(m.group(1)) == 512
    assert abi.FRAME_OUT_SPLIT == 512
    assert re.search(r"pub const AIC_FRAME_OUT_SPLIT: u32 = 512;", FFI)
    # a bit of its own among the frame flags
    others = [abi.FRAME_COUNTERS, abi.FRAME_AUX, abi.FRAME_PIXEL_CENTERS, abi.FRAME_OUT_LINEAR, abi.FRAME_OUT_COLORBUF, abi.FRAME_NO_FEEDBACK, abi.FRAME_BLOOM]
    assert all(abi.FRAME_OUT_SPLIT & o == 0 for o in others)
    assert abi.load().aic_abi_version() == 3  # backward compatible: the ABI version stays


def test_entry_points_are_declared_bound_and_exported():
    assert re.search(r"int aic_set_depth_transform\(aic_ctx \*ctx, const double zw\[4\]\);", HEADER)
    assert re.search(r"int aic_multi_set_depth_transform\(aic_multi \*m, const double zw\[4\]\);", HEADER)
    assert re.search(r"pub fn aic_set_depth_transform\(ctx: \*mut aic_ctx, zw: \*const f64\) -> c_int;", FFI)
    assert re.search(r"pub fn aic_multi_set_depth_transform\(m: \*mut aic_multi, zw: \*const f64\) -> c_int;", FFI)
    assert "pub fn draw_split" in SHIM and "AIC_FRAME_OUT_SPLIT" in SHIM and "aic_set_depth_transform" in SHIM
    lib = abi.load()
    for name in ("aic_set_depth_transform", "aic_multi_set_depth_transform"):
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(abi.Context, "set_depth_transform") and hasattr(abi.MultiContext, "set_depth_transform")
    assert hasattr(H.HipRtRenderer, "draw_split") and hasattr(H.Camera, "depth_transform_zw")
    # a null context is rejected, not dereferenced (the library needs no device for that)
    lib.aic_set_depth_transform.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    assert lib.aic_set_depth_transform(None, (C.c_double * 4)(1, 0, 0, 1)) == 1  # AIC_ERR_INVALID


def test_split_planes_views_the_two_planes():
    rows, w = 3, 5
    n = rows * w
    color = np.arange(n * 4, dtype=np.float16).reshape(rows, w, 4)
    depth = -np.arange(n, dtype=np.float32).reshape(rows, w)
    raw = np.concatenate([color.reshape(-1).view(np.uint8), depth.reshape(-1).view(np.uint8)])
    got = abi.split_planes(raw, rows, w)
    assert got["color_f16"].dtype == np.float16 and got["color_f16"].shape == (rows, w, 4)
    assert got["depth"].dtype == np.float32 and got["depth"].shape == (rows, w)
    assert (got["color_f16"].view(np.uint16) == color.view(np.uint16)).all()
    assert (got["depth"].view(np.uint32) == depth.view(np.uint32)).all()
    with pytest.raises(ValueError):
        abi.split_planes(raw[:-1], rows, w)


def depth_transform_zw_restated(projection, view_distance: float) -> np.ndarray:
    """{s P33, b P33 + P43, s P34, b P34 + P44} in numpy f64, one rounding per operation: P pre-translated by b = -near along z and pre-scaled by
    s = -(far - near), near = 1/32, far = the view distance."""
    p = np.asarray(projection, np.float64)
    near, far = np.float64(1.0 / 32.0), np.float64(view_distance)
    s = -(far - near)
    b = -near
    p33, p34, p43, p44 = p[2, 2], p[2, 3], p[3, 2], p[3, 3]
    return np.array([s * p33, b * p33 + p43, s * p34, b * p34 + p44], np.float64)


@pytest.mark.parametrize("fov_y", [90.0, 60.0])
@pytest.mark.parametrize("view_distance", [1.0, 200.0, 10000.0])
def test_depth_transform_zw_is_the_restated_formula_bit_for_bit(view_distance, fov_y):
    w, h = 40, 24
    o = H.GraphicsOptions()
    o.view_distance = view_distance
    o.fov_y = fov_y
    cam = H.Camera(o, H.Viewport.with_scale(1.0, w, h))
    projection, _, _ = oracle.camera_matrices(fov_y, view_distance, w / h)
    want = depth_transform_zw_restated(projection, view_distance)
    got = np.array(cam.depth_transform_zw(), np.float64)
    assert (got.view(np.uint64) == want.view(np.uint64)).all(), (got, want)
    # what it is for: t = 0 (the near plane) projects to depth 0, t = 1 (the view distance) to depth 1
    z0, w0 = want[1], want[3]
    z1, w1 = want[0] + want[1], want[2] + want[3]
    assert abs(z0 / w0) < 1e-12 and abs(z1 / w1 - 1.0) < 1e-9
