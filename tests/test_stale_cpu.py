"""CPU tests of the stale-pixel rule: aic_stale_rects against tests/stale_ref.py field for field, the rule's conservativeness against
the oracle -- every pixel outside the stale set is byte-identical before and after the edit --, and the helper's rejections. No device is needed."""
import ctypes as C

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from tests import stale_ref
from tests import stale_scenes as S

AIC_ERR_INVALID = 1
SIZES = [(1, 1), (61, 37), (96, 64)]
EXPANDS = [0, 1, 3]


def perspective(rng, w, h):
    eye = rng.uniform(-20.0, 20.0, 3)
    target = eye + rng.uniform(-1.0, 1.0, 3) * (1.0, 0.6, 1.0) + (0.0, 0.0, 1e-3)
    projection, world_to_eye, _ = oracle.camera_matrices(float(rng.choice([45.0, 90.0, 120.0])), 200.0, w / h, oracle.look_at_y_up(eye, target), eye)
    return (world_to_eye @ projection).reshape(16), eye, target


def orthographic():
    """w = 1 everywhere: x and y scaled to a 24 x 16 window around (3, 2), z from [-40, 40] to [0, 1]; column-major"""
    m = np.zeros((4, 4))  # [c][r]
    m[0][0], m[1][1], m[2][2], m[3][3] = 1.0 / 12.0, 1.0 / 8.0, 1.0 / 80.0, 1.0
    m[3][0], m[3][1], m[3][2] = -3.0 / 12.0, -2.0 / 8.0, 0.5
    return m.reshape(16)


def boxes_around(rng, eye, target):
    """in front of the camera, straddling the camera plane, behind it, off-screen, of no volume, at the i32 edges"""
    eye, fwd = np.asarray(eye), np.asarray(target) - np.asarray(eye)
    fwd = fwd / np.linalg.norm(fwd)
    side = np.cross(fwd, (0.0, 1.0, 0.0))
    out = []
    for centre, half in [(eye + 12 * fwd, 1), (eye + 30 * fwd, 3), (eye + 3 * fwd, 1), (eye, 2), (eye + 1 * fwd, 4), (eye - 10 * fwd, 2),
                         (eye + 5 * fwd + 60 * side, 1), (eye + 5 * fwd + (0, 80, 0), 1)]:
        lo = np.floor(centre).astype(np.int64) - half + rng.integers(0, 2, 3)
        out.append([*lo, *(lo + 2 * half)])
    lo = np.floor(eye + 12 * fwd).astype(np.int64)
    out += [[*lo, lo[0], lo[1] + 1, lo[2] + 1], [*lo, lo[0] + 1, lo[1] - 2, lo[2] + 1], [*lo, *lo]]  # no volume
    out += [[-2**31, -2**31, -2**31, 2**31 - 1, 2**31 - 1, 2**31 - 1], [2**31 - 3, 0, 0, 2**31 - 1, 1, 1], [-2**31, 0, 0, -2**31 + 2, 1, 1]]
    return np.array(out, np.int32)


def test_rects_equal_the_restatement_field_for_field():
    rng = np.random.default_rng(20)
    kinds = {"whole": 0, "empty": 0, "proper": 0}
    for w, h in SIZES:
        cams = [perspective(rng, w, h) for _ in range(6)] + [(orthographic(), (3.0, 2.0, -10.0), (3.0, 2.0, 0.0))]
        for vp, eye, target in cams:
            b = boxes_around(rng, eye, target)
            for expand in EXPANDS:
                got = abi.stale_rects(vp, w, h, b, expand)
                want = stale_ref.rects(vp, w, h, b, expand)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (w, h, expand, got[got != want][:3], want[got != want][:3])
                for r in want:
                    whole = (r["x1"], r["y1"]) == (w, h) and (r["x0"], r["y0"]) == (0, 0) and r["dmin"] == -np.inf
                    empty = r["x1"] == 0 and r["y1"] == 0
                    kinds["whole" if whole else ("empty" if empty else "proper")] += 1
                    assert r["x0"] <= r["x1"] <= w and r["y0"] <= r["y1"] <= h and not np.isnan(r["dmin"]) and r["reserved"] == 0
    print(kinds)
    assert all(v > 20 for v in kinds.values()), kinds
    assert len(abi.stale_rects(orthographic(), 5, 5, np.zeros((0, 6), np.int32))) == 0


def frames_differ(a, b):
    return (a[0].view(np.uint64).reshape(-1) != b[0].view(np.uint64).reshape(-1)) | (a[1].view(np.uint32).reshape(-1) != b[1].view(np.uint32).reshape(-1))


@pytest.mark.parametrize("antialiasing", S.ANTIALIASING)
@pytest.mark.parametrize("name", S.CASES)
def test_pixels_outside_the_stale_set_do_not_change(name, antialiasing):
    """The oracle's Split frames of A and of B = A with cubes removed, added beside a lit surface and swapped for a recursive block, the light volume
    unchanged: every pixel outside S (expand = 1) holds the same bytes in both. S is at most half the frame, so the rule cannot pass by marking all."""
    a, b = S.oracle_split(name, "A", antialiasing), S.oracle_split(name, "B", antialiasing)
    differ = frames_differ(a, b)
    s, rects = S.stale_set(name, antialiasing, 0)
    print(f"{name} aa {antialiasing}: {int(differ.sum())} pixels differ, n_stale {int(s.sum())} of {S.W * S.HT}, rects {rects.tolist()}")
    assert differ.sum() >= 20, "the edit shows"
    assert s.sum() <= S.W * S.HT // 2
    assert not (differ & ~s).any()
    assert (stale_ref.rank_list(s, None) == np.flatnonzero(s)).all()


@pytest.mark.parametrize("antialiasing", S.ANTIALIASING)
def test_depth_test_keeps_the_pixels_in_front_out_and_stays_conservative(antialiasing):
    """behind_wall is opaque only and one changed cube is hidden behind a wall: with AIC_STALE_DEPTH_TEST the wall's pixels inside that cube's rectangle are
    kept out, S_depth is a proper subset of S_plain, and still no pixel outside it changes. This is what judges the dmin margin."""
    name = "behind_wall"
    a, b = S.oracle_split(name, "A", antialiasing), S.oracle_split(name, "B", antialiasing)
    differ = frames_differ(a, b)
    plain, rects = S.stale_set(name, antialiasing, 0)
    deep, _ = S.stale_set(name, antialiasing, stale_ref.DEPTH_TEST)
    alpha = a[0][..., 3].view(np.float16)
    assert (alpha == 1.0).all(), "opaque only"
    print(f"{name} aa {antialiasing}: {int(differ.sum())} pixels differ, S_plain {int(plain.sum())}, S_depth {int(deep.sum())}")
    assert differ.sum() >= 20
    assert not (deep & ~plain).any() and deep.sum() < plain.sum() <= S.W * S.HT // 2
    assert not (differ & ~deep).any()
    # the hidden cube's rectangle is where pixels were kept out, and the cube in front keeps all of its own
    hidden, front = rects[0], rects[1]
    kept_out = (plain & ~deep).reshape(S.HT, S.W)
    assert kept_out[hidden["y0"]:hidden["y1"], hidden["x0"]:hidden["x1"]].sum() == kept_out.sum()
    assert hidden["dmin"] > front["dmin"]


def test_rejections_of_the_helper():
    lib = abi.load()
    abi.stale_rects(orthographic(), 4, 4, [[0, 0, 0, 1, 1, 1]])  # (declares the argtypes)
    vp = (C.c_double * 16)(*orthographic())
    box = (C.c_int32 * 6)(0, 0, 0, 1, 1, 1)
    out = abi.StaleRect()
    sentinel = bytes([0xA5]) * C.sizeof(out)

    def call(m=vp, w=8, h=8, n=1, boxes=box, expand=1, dst=None):
        C.memmove(C.byref(out), sentinel, len(sentinel))
        return lib.aic_stale_rects(m, w, h, n, boxes, expand, C.byref(out) if dst is None else dst)

    assert call() == 0 and bytes(out) != sentinel
    for what, rc in [("NULL matrix", call(m=None)), ("NULL boxes", call(boxes=None)), ("NULL out", call(dst=C.c_void_p(None))), ("negative expand", call(expand=-1)),
                     ("width above 65535", call(w=65536)), ("height above 65535", call(h=65536))]:
        assert rc == AIC_ERR_INVALID, what
        assert bytes(out) == sentinel, what
    for bad in (np.nan, np.inf, -np.inf):
        for i in (0, 7, 15):
            m = (C.c_double * 16)(*orthographic())
            m[i] = bad
            assert call(m=m) == AIC_ERR_INVALID and bytes(out) == sentinel
    # n_boxes = 0 needs neither list; the largest frame is fine
    assert lib.aic_stale_rects(vp, 8, 8, 0, None, 1, None) == 0
    assert call(w=65535, h=65535) == 0
    with pytest.raises(abi.AicError):
        abi.stale_rects(orthographic(), 8, 8, [[0, 0, 0, 1, 1, 1]], expand=-2)
