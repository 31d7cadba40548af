"""aic_present_split_lines without a device: the structs against the header, the restatement (tests/present_lines_ref.py) on cases worked
by hand, aic_cursor_wireframe against vertices written out by hand and against a Python restatement of impl Wireframe for Cursor, and the condition
that makes the GPU test's cases worth running: in each, some fragments pass the depth test, some are hidden, and pixels are contested."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from all_is_cubes_amd import abi
from tests import present_lines_cases as cases
from tests import present_lines_ref as ref
from tests import reproject_ref

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
IDENTITY = np.eye(4, dtype=F).reshape(16)
ONE = np.array([1.0], F).view(np.uint32)[0]


def test_structs_match_the_header():
    """sizeof and offsetof as a C compiler reads include/aic_hip.h, against the ctypes mirrors."""
    structs = {"aic_line_vertex": None, "aic_lines_desc": abi.LinesDesc, "aic_lines_info": abi.LinesInfo, "aic_cursor_desc": abi.CursorDesc}
    fields = {"aic_line_vertex": ["position", "color"], **{name: [f[0] for f in t._fields_] for name, t in structs.items() if t}}
    prints = "".join(f'printf("{name} %zu", sizeof({name}));' + "".join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields[name]) + 'printf("\\n");'
                     for name in structs)
    d = tempfile.mkdtemp(prefix="aic_lines_structs_")
    src = os.path.join(d, "s.c")
    Path(src).write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "aic_hip.h"\nint main(void) {{ {prints} return 0; }}\n')
    subprocess.run(["cc", "-I", str(ROOT / "include"), src, "-o", os.path.join(d, "s")], check=True)
    out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out if line}
    assert seen["aic_line_vertex"] == [28, 0, 12] == [abi.LINE_VERTEX_DTYPE.itemsize, abi.LINE_VERTEX_DTYPE.fields["position"][1], abi.LINE_VERTEX_DTYPE.fields["color"][1]]
    for name, t in structs.items():
        if t:
            assert seen[name] == [C.sizeof(t)] + [getattr(t, f).offset for f in fields[name]], name
    assert (C.sizeof(abi.LinesDesc), C.sizeof(abi.LinesInfo), C.sizeof(abi.CursorDesc)) == (80, 32, 88)
    assert (abi.LINES_DEVICE, abi.LINES_MAX, abi.CURSOR_MAX_LINES) == (1, 1 << 20, 28)


def ndc(sx, sy, w, h):
    return sx / w * 2.0 - 1.0, 1.0 - sy / h * 2.0


def vertex(sx, sy, z, w, h, colour=(1.0, 2.0, 3.0)):
    """under the identity matrix: the vertex that lands at window position (sx, sy) with depth z"""
    return [*ndc(sx, sy, w, h), z, *colour, 1.0]


def drawn(w, h, lines, depth=None, m=IDENTITY):
    """(owner [h][w], S', counts) of `lines` over a black scene whose depth plane is 1.0 unless given"""
    s = np.zeros((h, w, 4), F)
    s[..., 3] = 1.0
    depth = np.full((h, w), ONE, np.uint32) if depth is None else np.asarray(depth, F).view(np.uint32).reshape(h, w)
    stats = {}
    out, counts = ref.draw(s, depth, np.array(lines, F).reshape(-1, 7), m, stats)
    return stats["owner"], out, counts


def test_a_horizontal_line_covers_the_centres_in_its_half_open_range():
    w, h = 4, 1
    owner, out, counts = drawn(w, h, [vertex(0.5, 0.5, 0.5, w, h), vertex(2.5, 0.5, 0.5, w, h)])
    assert owner.tolist() == [[0, 0, -1, -1]]  # centres 0.5 and 1.5 lie in [0.5, 2.5); 2.5 does not
    assert counts == {"n_clipped_away": 0, "n_fragments": 2, "n_passed": 2, "n_pixels": 2}
    assert out[0, :2, :3].tolist() == [[1.0, 2.0, 3.0]] * 2 and (out[0, 2:, :3] == 0).all() and (out[..., 3] == 1).all()
    # the same line given end first: the same pixels
    owner, _, _ = drawn(w, h, [vertex(2.5, 0.5, 0.5, w, h), vertex(0.5, 0.5, 0.5, w, h)])
    assert owner.tolist() == [[0, 0, -1, -1]]
    # ends just short of and just past a centre
    owner, _, _ = drawn(w, h, [vertex(0.75, 0.5, 0.5, w, h), vertex(2.75, 0.5, 0.5, w, h)])
    assert owner.tolist() == [[-1, 0, 0, -1]]
    # a zero-length line draws nothing, on a centre or off it
    for sx in (1.5, 1.25):
        owner, _, counts = drawn(w, h, [vertex(sx, 0.5, 0.5, w, h), vertex(sx, 0.5, 0.5, w, h)])
        assert (owner == -1).all() and counts["n_fragments"] == 0 and counts["n_clipped_away"] == 0


def test_at_45_degrees_the_major_axis_is_x():
    w = h = 4
    owner, _, counts = drawn(w, h, [vertex(0.0, 0.5, 0.5, w, h), vertex(3.0, 3.5, 0.5, w, h)])
    # x-major: centres 0.5, 1.5, 2.5 in [0, 3), rows floor(0.5 + t 3) = 1, 2, 3. (y-major would give (0, 0), (1, 1), (2, 2).)
    assert sorted(zip(*np.nonzero(owner == 0))) == [(1, 0), (2, 1), (3, 2)] and counts["n_fragments"] == 3
    owner, _, _ = drawn(w, h, [vertex(0.0, 0.0, 0.5, w, h), vertex(4.0, 4.0, 0.5, w, h)])
    assert sorted(zip(*np.nonzero(owner == 0))) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    # steeper than 45 degrees: y-major, one fragment a row
    owner, _, _ = drawn(w, h, [vertex(0.5, 0.0, 0.5, w, h), vertex(1.5, 4.0, 0.5, w, h)])
    assert sorted(zip(*np.nonzero(owner == 0))) == [(0, 0), (1, 0), (2, 1), (3, 1)]


def test_a_line_crossing_w_0_is_clipped_at_the_near_plane():
    w = h = 4
    m = reproject_ref.perspective(90.0, 1.0, 1.0, 10.0).T.reshape(16).astype(F)
    a, b = [-1.0, 0.0, -2.0, 1, 1, 1, 1], [3.0, 0.0, 2.0, 1, 1, 1, 1]  # in front of the eye, and behind it: w = 2 and w = -2
    seg = ref.segment(a, b, m, w, h)
    # a is at window x = 1; the near plane z = -1 is reached a quarter of the way, at window x = 2 with depth 0
    assert seg["x_major"] and seg["p"][0] == F(1.0) and abs(seg["p"][1] - 2.0) < 1e-5 and abs(seg["d"][1]) < 1e-6 and abs(seg["d"][0] - 5.0 / 9.0) < 1e-6
    owner, _, counts = drawn(w, h, [a, b], m=m)
    assert sorted(zip(*np.nonzero(owner == 0))) == [(2, 1)] and counts["n_fragments"] == 1
    owner_reversed, _, _ = drawn(w, h, [b, a], m=m)
    assert (owner_reversed == owner).all()
    # wholly behind the eye, wholly beyond a side, a non-finite vertex: dropped
    for line in ([[0, 0, 1.0, 1, 1, 1, 1], [1, 0, 2.0, 1, 1, 1, 1]], [[5.0, 0, -2.0, 1, 1, 1, 1], [9.0, 0, -2.0, 1, 1, 1, 1]],
                 [[0, 0, -2.0, 1, 1, 1, 1], [np.nan, 0, -2.0, 1, 1, 1, 1]], [[0, 0, -2.0, 1, np.inf, 1, 1], [1, 0, -2.0, 1, 1, 1, 1]]):
        owner, _, counts = drawn(w, h, line, m=m)
        assert (owner == -1).all() and counts == {"n_clipped_away": 1, "n_fragments": 0, "n_passed": 0, "n_pixels": 0}
    # alpha is never read: whatever it holds, the line is drawn
    for alpha in (np.nan, np.inf, -3.0):
        owner_alpha, _, _ = drawn(w, h, [a[:6] + [alpha], b[:6] + [alpha]], m=m)
        assert (owner_alpha == owner_reversed).all()


def test_of_two_lines_at_equal_depth_the_lower_index_shows_and_the_nearer_wins():
    w = h = 4
    across = [vertex(0.0, 1.5, 0.5, w, h, (1, 0, 0)), vertex(4.0, 1.5, 0.5, w, h, (1, 0, 0))]
    down = [vertex(2.5, 0.0, 0.5, w, h, (0, 1, 0)), vertex(2.5, 4.0, 0.5, w, h, (0, 1, 0))]
    for first, second, colour in ((across, down, [1, 0, 0]), (down, across, [0, 1, 0])):
        owner, out, counts = drawn(w, h, first + second)
        assert owner[1, 2] == 0 and out[1, 2, :3].tolist() == colour
        assert counts == {"n_clipped_away": 0, "n_fragments": 8, "n_passed": 8, "n_pixels": 7}
    nearer = [vertex(2.5, 0.0, 0.25, w, h, (0, 1, 0)), vertex(2.5, 4.0, 0.25, w, h, (0, 1, 0))]
    owner, out, _ = drawn(w, h, across + nearer)
    assert owner[1, 2] == 1 and out[1, 2, :3].tolist() == [0, 1, 0]
    # a two-coloured line is interpolated along the screen: t = 1/8, 3/8, 5/8, 7/8
    owner, out, _ = drawn(w, h, [vertex(0.0, 0.5, 0.5, w, h, (0, 0, 8)), vertex(4.0, 0.5, 0.5, w, h, (8, 0, 0))])
    assert out[0, :, 0].tolist() == [1, 3, 5, 7] and out[0, :, 2].tolist() == [7, 5, 3, 1]


def test_which_depth_texels_hide_a_line():
    w, h = 6, 1
    line = [vertex(0.0, 0.5, 0.5, w, h), vertex(6.0, 0.5, 0.5, w, h)]
    owner, _, counts = drawn(w, h, line, depth=[-0.0, np.nan, 1.5, 0.5, 0.75, -0.25])
    assert owner.tolist() == [[-1, -1, 0, -1, 0, -1]]  # a set sign bit hides; NaN hides; above 1 admits; Less, so an equal depth hides
    assert counts == {"n_clipped_away": 0, "n_fragments": 6, "n_passed": 2, "n_pixels": 2}
    at_far = [vertex(0.0, 0.5, 1.0, w, h), vertex(6.0, 0.5, 1.0, w, h)]
    owner, _, counts = drawn(w, h, at_far, depth=[1.5, np.inf, 1.0, 2.0, 1.5, 1.5])
    assert (owner == -1).all() and counts["n_fragments"] == 6 and counts["n_passed"] == 0  # f = 1 is never below min(texel, 1)
    # a stretched frame: the nearest texel by the pixel centre, never a blend of two
    texels = ref.depth_texels(np.array([[0.25, -0.0, 0.75]], F).view(np.uint32), 6, 1).view(F)
    assert np.array_equal(np.signbit(texels), [[False, False, True, True, False, False]]) and texels[0, 0] == 0.25 and texels[0, 5] == 0.75
    assert ref.depth_texels(np.arange(12, dtype=np.uint32).reshape(3, 4), 2, 2).tolist() == [[1, 3], [9, 11]]


# ---- aic_cursor_wireframe

LO, HI = (0.99, 1.99, 2.99), (2.01, 3.01, 4.01)  # the block at (1, 2, 3) grown by 0.001 x 10
BY_HAND = [
    # the box, Aab::wireframe_points' order: four edges along z, four along y, four along x
    (0.99, 1.99, 2.99), (0.99, 1.99, 4.01), (0.99, 3.01, 2.99), (0.99, 3.01, 4.01), (2.01, 1.99, 2.99), (2.01, 1.99, 4.01), (2.01, 3.01, 2.99), (2.01, 3.01, 4.01),
    (0.99, 1.99, 2.99), (0.99, 3.01, 2.99), (0.99, 1.99, 4.01), (0.99, 3.01, 4.01), (2.01, 1.99, 2.99), (2.01, 3.01, 2.99), (2.01, 1.99, 4.01), (2.01, 3.01, 4.01),
    (0.99, 1.99, 2.99), (2.01, 1.99, 2.99), (0.99, 1.99, 4.01), (2.01, 1.99, 4.01), (0.99, 3.01, 2.99), (2.01, 3.01, 2.99), (0.99, 3.01, 4.01), (2.01, 3.01, 4.01),
    # the selected face NZ: the box shrunk by 1/128 = 0.0078125 in x and y, flat at z = 2.99 -- its z edges have no length
    (0.9978125, 1.9978125, 2.99), (0.9978125, 1.9978125, 2.99), (0.9978125, 3.0021875, 2.99), (0.9978125, 3.0021875, 2.99),
    (2.0021875, 1.9978125, 2.99), (2.0021875, 1.9978125, 2.99), (2.0021875, 3.0021875, 2.99), (2.0021875, 3.0021875, 2.99),
    (0.9978125, 1.9978125, 2.99), (0.9978125, 3.0021875, 2.99), (0.9978125, 1.9978125, 2.99), (0.9978125, 3.0021875, 2.99),
    (2.0021875, 1.9978125, 2.99), (2.0021875, 3.0021875, 2.99), (2.0021875, 1.9978125, 2.99), (2.0021875, 3.0021875, 2.99),
    (0.9978125, 1.9978125, 2.99), (2.0021875, 1.9978125, 2.99), (0.9978125, 1.9978125, 2.99), (2.0021875, 1.9978125, 2.99),
    (0.9978125, 3.0021875, 2.99), (2.0021875, 3.0021875, 2.99), (0.9978125, 3.0021875, 2.99), (2.0021875, 3.0021875, 2.99),
    # the diamond about (1.5, 2.5, 3 - 0.01): tips at 1/32 = 0.03125 towards +x, +y, -x, -y, as a loop
    (1.53125, 2.5, 2.99), (1.5, 2.53125, 2.99), (1.5, 2.53125, 2.99), (1.46875, 2.5, 2.99), (1.46875, 2.5, 2.99), (1.5, 2.46875, 2.99), (1.5, 2.46875, 2.99), (1.53125, 2.5, 2.99),
]


def test_cursor_wireframe_by_hand():
    v = abi.cursor_wireframe((1, 2, 3), 3, 3, (1.5, 2.5, 3.0), 10.0)
    assert len(BY_HAND) == 56 and v.shape == (56,)
    assert np.array_equal(v["position"], np.array(BY_HAND, np.float64).astype(F))
    assert (v["color"] == np.array([0, 0, 0, 1], F)).all()


# impl Wireframe for Cursor (cursor.rs:219-278) in Python floats (f64), with the reference's names
OCTANTS = {"Nnn": (0, 0, 0), "Nnp": (0, 0, 1), "Npn": (0, 1, 0), "Npp": (0, 1, 1), "Pnn": (1, 0, 0), "Pnp": (1, 0, 1), "Ppn": (1, 1, 0), "Ppp": (1, 1, 1)}
WIREFRAME = [("Nnn", "Nnp"), ("Npn", "Npp"), ("Pnn", "Pnp"), ("Ppn", "Ppp"), ("Nnn", "Npn"), ("Nnp", "Npp"), ("Pnn", "Ppn"), ("Pnp", "Ppp"),
             ("Nnn", "Pnn"), ("Nnp", "Pnp"), ("Npn", "Ppn"), ("Npp", "Ppp")]
FACE_VECTORS = {0: (0, 0, 0), 1: (-1, 0, 0), 2: (0, -1, 0), 3: (0, 0, -1), 4: (1, 0, 0), 5: (0, 1, 0), 6: (0, 0, 1)}  # Face7 discriminants
# Face::rotation_from_nz (face.rs:395-405) as the faces its basis sends +X, +Y, +Z to: RYZX, RZXY, RXYZ, RyZx, RZxy, RXyz
ROTATION_FROM_NZ = {1: (5, 6, 4), 2: (6, 4, 5), 3: (4, 5, 6), 4: (2, 6, 1), 5: (6, 1, 2), 6: (4, 2, 3)}


def wireframe_restated(cube, face_entered, face_selected, point, distance, lo, size, resolution):
    offset = 0.001 * distance
    recip = 1.0 / resolution
    low = [lo[a] * recip + cube[a] - offset for a in range(3)]
    high = [(lo[a] + size[a]) * recip + cube[a] + offset for a in range(3)]
    def box(low, high):
        return [tuple((low, high)[OCTANTS[corner][a]][a] for a in range(3)) for edge in WIREFRAME for corner in edge]
    out = box(low, high)
    if face_selected:
        inset = -1.0 / 128.0
        f_low, f_high = [v - inset for v in low], [v + inset for v in high]
        axis = (face_selected - 1) % 3
        f_low[axis] = f_high[axis] = low[axis] if face_selected <= 3 else high[axis]
        out += box(f_low, f_high)
    if face_entered:
        basis = [FACE_VECTORS[f] for f in ROTATION_FROM_NZ[face_entered]]
        tips = []
        for f in (4, 5, 1, 2):  # Face7::PX, PY, NX, NY
            vec = [c / 32.0 for c in FACE_VECTORS[f]]
            tip = [vec[0] * basis[0][a] + vec[1] * basis[1][a] + vec[2] * basis[2][a] for a in range(3)]
            tips.append(tuple(point[a] + FACE_VECTORS[face_entered][a] * offset + tip[a] for a in range(3)))
        out += [tips[(k + end) % 4] for k in range(4) for end in range(2)]
    return np.array(out, np.float64).astype(F)


def test_cursor_wireframe_equals_its_restatement():
    blocks = [((1, 2, 3), (0, 0, 0), (1, 1, 1), 1), ((-7, 0, 40), (2, 0, 5), (9, 16, 3), 16), ((0, 0, 0), (0, 3, 0), (4, 1, 4), 4)]
    for (cube, lo, size, resolution), entered, selected in itertools.product(blocks, range(7), range(7)):
        point = (cube[0] + 0.3, cube[1] + 0.55, cube[2] + 0.8125)
        got = abi.cursor_wireframe(cube, entered, selected, point, 3.7, lo, size, resolution)
        want = wireframe_restated(cube, entered, selected, point, 3.7, lo, size, resolution)
        assert len(got) == 2 * (12 + (12 if selected else 0) + (4 if entered else 0))
        assert np.array_equal(got["position"].view(np.uint32), want.view(np.uint32)), (cube, entered, selected)
    # a resolution-16 block with a partial voxel box: x from 2/16 to 11/16 of the cube at -7, grown by 0.0037
    v = abi.cursor_wireframe((-7, 0, 40), 0, 0, (0, 0, 0), 3.7, (2, 0, 5), (9, 16, 3), 16)
    assert len(v) == 24
    assert v["position"][:, 0].min() == F(-7 + 2 / 16 - 0.0037) and v["position"][:, 0].max() == F(-7 + 11 / 16 + 0.0037)
    assert v["position"][:, 2].min() == F(40 + 5 / 16 - 0.0037) and v["position"][:, 2].max() == F(40 + 8 / 16 + 0.0037)
    assert [len(abi.cursor_wireframe((0, 0, 0), e, s, (0, 0, 0), 1.0)) // 2 for e, s in ((0, 0), (2, 0), (0, 5), (6, 1))] == [12, 16, 24, 28]
    for bad in ({"face_entered": 7}, {"face_selected": -1}, {"resolution": 0}, {"voxel_size": (1, -1, 1)}):
        kw = {"cube": (0, 0, 0), "face_entered": 0, "face_selected": 0, "point_entered": (0, 0, 0), "distance_to_point": 1.0, **bad}
        with pytest.raises(abi.AicError):
            abi.cursor_wireframe(**kw)


# ---- the GPU test's cases

@pytest.mark.parametrize("src_size,out_size", cases.SIZES)
def test_the_gpu_cases_hide_some_fragments_pass_others_and_contest_pixels(src_size, out_size):
    """From the restatement alone: 1 <= n_passed < n_fragments and a contested pixel, in every case that can have them. Two kinds of case cannot, and
    are held to what they can show instead: a list of ONE line has one fragment per major index, so no pixel of it is contested (asserted: some of its
    fragments pass and some are hidden); and one line in a window of ONE pixel has one fragment (asserted: it passes). Nothing else is waived."""
    for n in cases.N_LINES:
        _, depth, vertices, _, parts, stats = cases.restated(src_size, out_size, n)
        counts = parts["counts"]
        what = (src_size, out_size, n, counts, stats["contested"], stats["ties"])
        assert counts["n_pixels"] >= 1 and counts["n_pixels"] <= counts["n_passed"], what
        if n == 1:
            assert counts["n_clipped_away"] == 0 and counts["n_fragments"] >= min(out_size), what  # it crosses the whole window
            assert counts["n_passed"] == 1 if out_size == (1, 1) else 1 <= counts["n_passed"] < counts["n_fragments"], what
            continue
        assert 1 <= counts["n_passed"] < counts["n_fragments"], what
        assert stats["contested"] >= 1, what
        assert 1 <= counts["n_clipped_away"] < n, what
    texels = np.asarray(cases.synthetic_frame(*src_size)[1]).view(F)
    if src_size[0] * src_size[1] >= 64 * 48:  # every kind of depth texel is there
        assert ((texels > 0) & (texels < 1)).any() and (texels == 1).any() and (texels > 1).any() and np.isnan(texels).any()
        assert (np.signbit(texels) & (texels == 0)).any() and (texels < 0).any()


def test_the_lists_hold_every_kind_of_line():
    w, h = 64, 48
    v = cases.line_list(1000, w, h).reshape(-1, 2, 7)
    m = cases.view_projection(w, h)
    segs = [ref.segment(a, b, m, w, h) for a, b in v]
    assert np.isnan(v).sum() == 1
    assert any((a[:3] == b[:3]).all() for a, b in v) and any((a[3:6] != b[3:6]).any() for a, b in v)
    assert any((v[k] == v[k - 7])[..., :3].all() and (v[k] != v[k - 7])[..., 3:6].any() for k in range(7, 1000))
    w_of = lambda p: m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15]
    assert any(s is not None and min(w_of(a), w_of(b)) < 0 for s, (a, b) in zip(segs, v))  # crosses w = 0 and still shows
    flat = [s for s in segs if s is not None and s["q"][0] == s["q"][1]]
    diagonal = [s for s in segs if s is not None and abs(abs(s["p"][1] - s["p"][0]) - abs(s["q"][1] - s["q"][0])) < 1e-3 and s["p"][1] - s["p"][0] > 1]
    centred = [s for s in segs if s is not None and abs(s["p"][0] % 1 - 0.5) < 1e-3 and abs(s["p"][1] % 1 - 0.5) < 1e-3]
    assert flat and diagonal and centred
