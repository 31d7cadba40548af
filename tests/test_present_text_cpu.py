"""The info text of a presentation without a device (aic_set_text_font, aic_text_geometry, aic_text_layout, aic_present_split_text):
the host-only entry points against the restatement (tests/present_text_ref.py), the structs and names across the layers, the host mirror's font atlas
against draw_info_text -- the routine the info_text goldens pin --, and the restatement itself on a window worked by hand and against draw_info_text."""
import ctypes as C
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import present_ref
from tests import present_text_ref as ref

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
NOMINALS = [(1, 1), (7, 16), (8, 17), (640.5, 480.25), (1920, 1080), (65535, 1)]
CELLS = [(9, 18, 1), (5, 7, 0), (3, 3, 1)]
BLACK, WHITE = (0, 0, 0, 255), (255, 255, 255, 255)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("nominal", NOMINALS)
def test_geometry_equals_the_restatement(nominal, cell):
    cols, rows, scale, origin = abi.text_geometry(nominal, cell)
    want = ref.geometry(nominal, cell)
    assert (cols, rows) == want[:2]
    assert scale.dtype == F and (scale.view(np.uint32) == want[2].view(np.uint32)).all()
    assert (origin.view(np.uint32) == want[3].view(np.uint32)).all()
    logical = (cell[0] - 2 * cell[2], cell[1] - 2 * cell[2])
    assert (cols - 1) * logical[0] < nominal[0] <= cols * logical[0] and (rows - 1) * logical[1] < nominal[1] <= rows * logical[1]  # the grid just covers the viewport


def test_geometry_by_hand_and_its_rejections():
    cols, rows, scale, origin = abi.text_geometry((1920, 1080), (9, 18, 1))
    assert (cols, rows) == (275, 68)  # ceil(1920 / 7), ceil(1080 / 16)
    assert scale[0] == F(1920) / F(1925) and scale[1] == F(1080) / F(1088)
    assert origin[0] == F(5 / 1920) and origin[1] == F(5 / 1080)
    bad = [((0, 1), (9, 18, 1)), ((1, -1), (9, 18, 1)), ((float("inf"), 1), (9, 18, 1)), ((1, float("nan")), (9, 18, 1)), ((8, 8), (0, 18, 1)), ((8, 8), (9, 1025, 1)),
           ((8, 8), (4, 18, 2)), ((8, 8), (9, 2, 1)), ((65536, 8), (3, 3, 1)), ((8, 65535.5), (3, 3, 1))]
    for nominal, cell in bad:
        assert ref.geometry(nominal, cell) is None, (nominal, cell)
        with pytest.raises(abi.AicError) as err:
            abi.text_geometry(nominal, cell)
        assert err.value.code == 1, (nominal, cell)
    assert abi.text_geometry((65535, 1), (3, 3, 1))[:2] == (65535, 1)


LAYOUTS = [("", 8, 3), ("\n\n\n", 8, 3), ("a line longer than the grid\nnext", 8, 3), ("1\n2\n3\n4\n5", 8, 3), ("é€“", 8, 3), (b"\xff\xc3", 8, 3), (b"a\x80b\xe2\x82", 8, 3),
           (b"\xf4\x90\x80\x80x\xed\xa0\x80y", 8, 3), ("a b\nc d", 8, 3), ("\x01\x7f\xa0\xff", 4, 1), ("ab\ncd", 1, 1), ("FPS 60.0\n12 ms\nrays 1e6", 275, 68)]


@pytest.mark.parametrize("text,cols,rows", LAYOUTS)
def test_layout_equals_the_restatement(text, cols, rows):
    codes, used = abi.text_layout(text, cols, rows)
    want, want_used = ref.layout(text, cols, rows)
    assert codes.shape == (rows, cols) and (codes == want).all() and used == want_used


def test_layout_by_hand_and_its_rejections():
    assert abi.text_layout("", 8, 3)[1] == (0, 0) and not abi.text_layout("\n\n", 8, 3)[0].any()
    codes, used = abi.text_layout("a line longer\nmore\n\nlines than rows", 6, 3)
    assert bytes(codes[0]) == b"a line" and bytes(codes[1]) == b"more\0\0" and not codes[2].any() and used == (6, 2)
    codes, used = abi.text_layout("é€x", 4, 1)
    assert bytes(codes[0]) == b"\xe9?x\0" and used == (3, 1)
    codes, used = abi.text_layout(b"\xffa\xc3", 4, 2)  # a stray byte, and a sequence the end cuts off: U+FFFD each
    assert bytes(codes[0]) == b"?a?\0" and used == (3, 1)
    codes, used = abi.text_layout("a\n\n  b", 4, 3)
    assert used == (3, 3) and bytes(codes[2]) == b"  b\0"
    for cols, rows in ((0, 1), (1, 0), (65536, 1), (1, 65536)):
        with pytest.raises(abi.AicError) as err:
            abi.text_layout("a", cols, rows)
        assert err.value.code == 1


def test_structs_match_the_header():
    """sizeof and offsetof as a C compiler reads include/aic_hip.h, against the ctypes mirror."""
    fields = [f[0] for f in abi.TextDesc._fields_]
    prints = 'printf("%zu", sizeof(aic_text_desc));' + "".join(f'printf(" %zu", offsetof(aic_text_desc, {f}));' for f in fields) + 'printf(" %u\\n", AIC_TEXT_DEVICE);'
    d = tempfile.mkdtemp(prefix="aic_text_structs_")
    src = os.path.join(d, "s.c")
    Path(src).write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "aic_hip.h"\nint main(void) {{ {prints} return 0; }}\n')
    subprocess.run(["cc", "-I", str(ROOT / "include"), src, "-o", os.path.join(d, "s")], check=True)
    seen = [int(v) for v in subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()]
    assert seen == [C.sizeof(abi.TextDesc)] + [getattr(abi.TextDesc, f).offset for f in fields] + [abi.TEXT_DEVICE]
    assert C.sizeof(abi.TextDesc) == 40


def test_every_layer_names_the_four_entry_points():
    names = ("aic_set_text_font", "aic_text_geometry", "aic_text_layout", "aic_present_split_text")
    lib = abi.load()
    texts = {rel: (ROOT / rel).read_text() for rel in ("include/aic_hip.h", "all_is_cubes_amd/abi.py", "all_is_cubes_amd/host/aic_host.cpp", "rust/all-is-cubes-hip/src/ffi.rs",
                                                        "rust/all-is-cubes-hip/src/lib.rs", "README.md", "INTEGRATION.md", "DESIGN.md")}
    for name in names:
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name)
        for rel, text in texts.items():
            assert name in text, (name, rel)
    assert "AIC_ABI_VERSION 3" in texts["include/aic_hip.h"]
    for attr in ("TextDesc", "text_geometry", "text_layout", "TEXT_DEVICE"):
        assert hasattr(abi, attr)
    assert hasattr(abi.Context, "set_text_font") and hasattr(abi.Context, "present_split_text")
    assert hasattr(H, "info_text_font_atlas") and hasattr(H.HipRtRenderer, "present_split_text") and H.INFO_TEXT_CELL == (9, 18, 1)


def test_the_mirror_atlas_is_draw_info_text_cell_by_cell():
    atlas = H.info_text_font_atlas()
    assert atlas.shape == (288, 144, 4) and atlas.dtype == np.uint8
    shown = 0
    for code in range(256):
        image = np.zeros((32, 32, 4), np.uint8)
        H.draw_info_text(image, chr(code), BLACK, WHITE)
        cell = atlas[code // 16 * 18:code // 16 * 18 + 18, code % 16 * 9:code % 16 * 9 + 9]
        assert (cell == image[4:22, 4:13]).all(), code
        outside = image.copy()
        outside[4:22, 4:13] = 0
        assert not outside.any(), code  # the whole drawing lies in the cell
        shown += bool(cell.any())
    assert not atlas[2 * 18:3 * 18, 0:9].any()  # cell 0x20
    assert shown >= 190  # the printable characters of ISO-8859-1 and '?' for the rest; space, no-break space and '\n' draw nothing
    values = {tuple(t) for t in atlas.reshape(-1, 4)}
    assert values == {(0, 0, 0, 0), BLACK, WHITE}


def test_a_window_worked_by_hand():
    """4 x 4 window, a 1 x 1 grid holding 'A', cells of (3, 3, 1): a logical cell of one texel and an outline of one. scale 2 and origin 1/4 put the
    logical cell over pixels 1 and 2 of each axis: tc = (u - 1/4) * 2 = -1/4, 1/4, 3/4, 5/4, every value exact. Pixel 0 reaches cell 0 at position
    -1/4: atlas texel floor(-1/4 * 1 + 1) = 0, the outline; pixels 1 and 2 at 1/4 and 3/4: texel 1; pixel 3 at 5/4: texel 2."""
    atlas = np.zeros((48, 48, 4), np.uint8)
    cell = np.array([[(0, 0, 0, 255), (0, 0, 0, 255), (0, 0, 0, 0)],
                     [(0, 0, 0, 255), (255, 255, 255, 255), (0, 0, 0, 255)],
                     [(0, 0, 0, 0), (0, 0, 0, 255), (51, 102, 153, 204)]], np.uint8)
    atlas[4 * 3:4 * 3 + 3, 1 * 3:1 * 3 + 3] = cell  # 'A' = 0x41
    atlas[2 * 3:2 * 3 + 3, 0:3] = 255  # (a space that is not blank: never read, the grid has no zero)
    text = ref.text_layer(4, 4, atlas, (3, 3, 1), np.array([[0x41]], np.uint8), (2.0, 2.0), (0.25, 0.25))
    t = [0, 1, 1, 2]
    want = np.array([[cell[t[y], t[x]] for x in range(4)] for y in range(4)], F) / F(255)
    assert (text == want).all()
    s = np.full((4, 4, 4), 0.5, F)
    out = ref.composite(s, None, 0.0, out_f16=True, text=text).view(np.float16).astype(F)
    k = F(1.0) - F(204) / F(255)
    corner = [np.float16(F(0.5) * k + F(c) / F(255)) for c in (51, 102, 153)]
    by_hand = {0: [0, 0, 0], 1: [1, 1, 1], 2: [0.5, 0.5, 0.5], 3: corner}  # outline, glyph, nothing, the translucent corner
    kinds = [[0, 0, 0, 2], [0, 1, 1, 0], [0, 1, 1, 0], [2, 0, 0, 3]]
    for y in range(4):
        for x in range(4):
            assert list(out[y, x, :3]) == [F(v) for v in by_hand[kinds[y][x]]] and out[y, x, 3] == 1.0, (x, y)
    # the same grid with a zero code reads the space
    blank = ref.text_layer(4, 4, atlas, (3, 3, 1), np.zeros((1, 1), np.uint8), (2.0, 2.0), (0.25, 0.25))
    assert (blank == 1.0).all()
    # a grid the window leaves: nothing
    assert not ref.text_layer(4, 4, atlas, (3, 3, 1), np.array([[0x41]], np.uint8), (2.0, 2.0), (4.0, -4.0)).any()


def background(w, h):
    rng = np.random.default_rng(100 * w + h)
    color = rng.exponential(0.3, (h, w, 4)).astype(np.float16).view(np.uint16)
    return present_ref.scene(color, w, h)


@pytest.mark.parametrize("size", [(64, 48), (97, 41), (1920, 40)])
def test_the_restatement_paints_what_draw_info_text_paints(size):
    """Isolated characters, so that no two glyph boxes meet and the host routine's last-glyph-wins is the shader's maximum; nominal size = window size."""
    w, h = size
    text = "a b\nc d"
    cols, rows, scale, origin = ref.geometry(size, H.INFO_TEXT_CELL)
    codes, _ = ref.layout(text, cols, rows)
    layer = ref.text_layer(w, h, H.info_text_font_atlas(), H.INFO_TEXT_CELL, codes, scale, origin)
    s = background(w, h)
    for tm, mi in ((0, np.inf), (1, 1.0)):
        got = ref.composite(s, None, 0.0, tm, mi, text=layer)
        want = present_ref.composite(s, None, 0.0, tm, mi).copy()
        plain = want.copy()
        H.draw_info_text(want, text, BLACK, WHITE)
        assert (want != plain).any(axis=-1).sum() >= 4 * 20
        assert (got == want).all()
    # at half the nominal size (a window of twice the pixels) every glyph texel covers 2 x 2 pixels
    layer2 = ref.text_layer(2 * w, 2 * h, H.info_text_font_atlas(), H.INFO_TEXT_CELL, codes, scale, origin)
    assert (layer2 == np.repeat(np.repeat(layer, 2, axis=0), 2, axis=1)).all()
