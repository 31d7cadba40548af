"""CPU-side checks of the reprojection post-process (aic_reproject_split): the chain's geometry as the library reports it, the host mirror's reprojection
matrix against a NumPy f64 construction, and the NumPy restatement (tests/reproject_ref.py) on cases whose result is known without it. No GPU."""
import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import reproject_ref as ref

SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (64, 48), (128, 256), (1920, 1080), (3840, 2160)]
STATED = {(64, 48): (6, (64, 64)), (128, 256): (8, (256, 256)), (1920, 1080): (11, (2048, 2048)), (3840, 2160): (12, (4096, 4096))}
F16_ONE = 0x3C00


def test_symbols_and_structs():
    assert {"aic_reproject_split", "aic_reproject_geometry"} <= set(abi.ABI_SYMBOLS)
    lib = abi.load()
    assert hasattr(lib, "aic_reproject_split") and hasattr(lib, "aic_reproject_geometry")
    import ctypes as C

    assert C.sizeof(abi.ReprojectDesc) == 8 + 64 + 16 + 8 and C.sizeof(abi.ReprojectInfo) == 48
    assert abi.REPROJECT_KEEP_SPLATS == 1 and abi.REPROJECT_MAX_LEVELS == 12 == ref.MAX_LEVELS


@pytest.mark.parametrize("w,h", SIZES)
def test_geometry_equals_the_restatement(w, h):
    got = abi.reproject_geometry(w, h)
    assert got == ref.geometry(w, h)
    if (w, h) in STATED:
        assert got[:2] == STATED[(w, h)]


def test_geometry_edges():
    assert abi.reproject_geometry(0, 7) == (0, (0, 0), 0) == ref.geometry(0, 7)
    assert abi.reproject_geometry(1920, 1080)[2] == 44362432  # the byte count include/aic_hip.h states
    assert abi.reproject_geometry(65535, 65535)[0] == 12
    for w, h in ((65536, 1), (1, 65536)):
        with pytest.raises(abi.AicError) as err:
            abi.reproject_geometry(w, h)
        assert err.value.code == 1


def camera(w, h, eye, target, fov=90.0):
    o = H.GraphicsOptions()
    o.fov_y = fov
    c = H.Camera(o, H.Viewport.with_scale(1.0, w, h))
    c.look_at_y_up(eye, target)
    return c


def mat(flat16):
    return np.array(flat16, np.float64).reshape(4, 4)  # euclid's row-vector matrices, m[row][col]


def test_reprojection_matrix_against_numpy():
    old = camera(128, 96, (0.7, 0.9, 2.5), (0.5, 0.5, 0.5))
    new = camera(128, 96, (0.9, 1.0, 2.3), (0.45, 0.5, 0.5))
    got = np.array(H.Camera.reprojection_matrix(old, new), np.float32)
    # raytrace_to_texture.rs:446-453 in row-vector order: then() is a product with the later transform on the right
    want = np.linalg.inv(mat(old.view_matrix()) @ mat(old.projection_matrix())) @ mat(new.view_matrix()) @ mat(new.projection_matrix())
    want = want.reshape(16).astype(np.float32)  # convert_matrix: euclid's rows are WGSL's columns, [c*4+r]
    scale = np.abs(want).max()
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-6 * scale
    same = np.array(H.Camera.reprojection_matrix(old, old), np.float64).reshape(4, 4)
    assert np.abs(same - np.eye(4)).max() <= 1e-6
    # the zw entries of the inverse projection
    ip = np.linalg.inv(mat(new.projection_matrix()))
    zw = np.array([ip[2, 2], ip[3, 2], ip[2, 3], ip[3, 3]])
    assert np.abs(np.array(new.inverse_projection_zw(), np.float64) - zw).max() <= 1e-6 * np.abs(zw).max()
    # a point of the old view lands where the new camera sees it: column-vector use of the column-major matrix
    m = got.reshape(4, 4).T.astype(np.float64)
    world = np.array([0.5, 0.5, 0.5, 1.0])
    clip_old = world @ mat(old.view_matrix()) @ mat(old.projection_matrix())
    clip_new = world @ mat(new.view_matrix()) @ mat(new.projection_matrix())
    through = m @ (clip_old / clip_old[3])
    assert np.abs(through / through[3] - clip_new / clip_new[3]).max() <= 1e-4


def random_color(rng, h, w):
    c = rng.integers(0, 0x7C00, (h, w, 4)).astype(np.uint16) | (rng.integers(0, 2, (h, w, 4)).astype(np.uint16) << 15)  # finite f16 of either sign
    c[..., 3] = rng.random((h, w)).astype(np.float16).view(np.uint16)
    return c


def test_identity_with_one_world_depth_copies_the_source():
    rng = np.random.default_rng(1)
    proj = ref.perspective(90.0, 24 / 16, 1 / 32, 200.0)
    m, zw = ref.reprojection(proj, ref.view(), ref.view())
    m = np.eye(4, dtype=np.float32).reshape(16)
    for w, h in ((24, 16), (64, 48)):  # every pixel against every sprite, and the boxed search
        color = random_color(rng, h, w)
        depth = np.full((h, w), 0.75, np.float32)
        out = ref.reproject(color, depth, m, zw)
        assert (out["R"] == color).all() and (out["D"].view(np.uint32) == depth.view(np.uint32)).all()
        assert (out["n_splats"], out["n_dropped"], out["n_gaps"], out["n_unfilled"]) == (w * h, 0, 0, 0)
        assert (ref.finish(out["R"], 1)["color"] == color).all()


def test_a_single_valid_texel_fills_the_image():
    R = np.tile(ref.MARKER, (8, 8, 1))
    R[5, 2] = np.array([0.25, 0.5, 2.0, 0.5], np.float16).view(np.uint16)
    for flags in (0, 1):
        out = ref.finish(R, flags)
        assert out["levels"] == 4 and out["t0"] == (16, 16) and out["n_unfilled"] == 0
        rgb = out["color"][..., :3].view(np.float16)
        assert (rgb == np.array([0.25, 0.5, 2.0], np.float16)).all()
        assert (np.delete(out["color"][..., 3].reshape(-1), 5 * 8 + 2) == F16_ONE).all()  # filled texels have alpha 1
    assert (ref.finish(R, 1)["color"][5, 2] == R[5, 2]).all()


def test_all_invalid_stays_invalid():
    R = np.tile(ref.MARKER, (9, 17, 1))
    out = ref.finish(R)
    assert (out["color"] == ref.MARKER).all() and out["n_unfilled"] == 17 * 9
    for _, _, mip in out["stages"]:
        assert (mip == ref.MARKER).all()


def test_depth_test_prefers_the_nearer_then_the_later_sprite():
    """Two equal depths tie towards the greater draw index; a nearer one wins whatever its index."""
    w, h = 6, 4
    proj = ref.perspective(90.0, w / h, 1 / 32, 200.0)
    _, zw = ref.reprojection(proj, ref.view(), ref.view())
    m = np.eye(4, dtype=np.float32).reshape(16)
    color = np.zeros((h, w, 4), np.uint16)
    color[..., 3] = F16_ONE
    color[..., 0] = np.arange(w * h, dtype=np.float16).reshape(h, w).view(np.uint16)
    depth = np.full((h, w), 0.5, np.float32)
    out = ref.splat(color, depth, m, zw)
    assert (out["R"] == color).all()  # each sprite's own pixel has d2 nearest 0 only for itself
    depth[1, 2] = 0.25
    out = ref.splat(color, depth, m, zw)
    near = out["R"][..., 0].view(np.float16) == np.float16(1 * w + 2)
    assert near[1, 2] and near.sum() > 1 and (out["D"][near] < 0.5).all()
