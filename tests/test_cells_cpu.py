"""The terminal's character cells without a GPU: the restatement (tests/cells_ref.py) against the reference's own known answers, the two context-free
entry points (aic_cells_geometry, aic_cells_ansi) against the restatement, and the edge images the GPU tests use."""
import ctypes as C
import itertools

import numpy as np
import pytest

from all_is_cubes_amd import abi
from tests import cells_ref as ref

MODE_PAIRS = list(itertools.product(ref.CHARACTER_MODES, ref.COLOR_MODES))


@pytest.mark.parametrize("characters, rows_of, want", [
    (ref.SHADES, "r", "  ░░▒▒▓▓██"),    # char_mode_shades
    (ref.SPLIT, "rr", "  ***▄▀███"),    # char_mode_split_same_luminance
    (ref.SHAPES, "rr", "  ░░▒▒▓▓██"),   # char_mode_shapes_same_luminance
    (ref.SHAPES, "br", "   ▁▁▂▂▃▃▄"),   # char_mode_split_upper
])
def test_the_references_known_answers(characters, rows_of, want):
    """chars.rs:350-404: the four tests of image_patch_to_character, every pixel's text '*'."""
    image = ref.ramp_image(rows_of)
    aux = np.zeros(image.shape[:2], abi.PIXEL_AUX_DTYPE)
    aux["hit"] = 1
    cells, _ = ref.cells(image, aux, 10, 1, characters, ref.COLOR_NONE)
    assert ref.glyph_text(cells[0]) == want


def test_cell_layout():
    assert abi.CELL_DTYPE.itemsize == 12 == ref.CELL_DTYPE.itemsize
    assert C.sizeof(abi.CellsDesc) == 32 and C.sizeof(abi.CellsInfo) == 72
    assert C.sizeof(abi.CellsText) == 2 * 8 + 2 * 8 + 8 + 4 + 4
    assert tuple(k for k, _ in abi.CellsInfo._fields_[1:16]) == ref.COUNTERS


@pytest.mark.parametrize("characters", ref.CHARACTER_MODES)
def test_geometry_matches_the_restatement(characters):
    for cols, rows in [(0, 0), (0, 1), (1, 0), (1, 1), (7, 5), (200, 60), (65535, 65535)]:  # options.rs:201-208 viewport_no_panic, and more
        assert abi.cells_geometry(cols, rows, characters) == ref.geometry(cols, rows, characters)


def test_geometry_rejections():
    for args in [(65536, 1, 0), (1, 65536, 0), (1, 1, 5), (1, 1, -1)]:
        with pytest.raises(abi.AicError) as e:
            abi.cells_geometry(*args)
        assert e.value.code == 1
    assert abi.load().aic_cells_geometry(3, 2, 4, None, None, None) == 0  # every output may be NULL


# names: one byte, several bytes, wide (2 columns), very wide, width 0, a missing entry
NAMES = (["a", "é", "漢", "wide", "́", None, "z"], ["U", "漢"])
WIDTHS = ([1, 1, 2, 4, 0, 1, 1], [1, 2])


def random_cells(rng, rows, cols):
    cells = np.zeros((rows, cols), ref.CELL_DTYPE)
    glyphs = np.array([0x20, ord("."), ord("X"), 0x2584, 0x2588, 0x28FF, 0x2591], np.uint32)
    colours = np.array([0, ref.RESET, ref.BLACK, (3 << 24) | 16, (3 << 24) | 231, (4 << 24) | 0x123456, (4 << 24) | 0xFFFFFF], np.uint32)
    cells["glyph"] = rng.choice(glyphs, (rows, cols))
    block = rng.random((rows, cols)) < 0.4
    refs = ref.GLYPH_BLOCK | (rng.integers(0, 2, (rows, cols)) << 16) | rng.integers(0, 9, (rows, cols))  # indices 7, 8 lie beyond the world's table
    cells["glyph"] = np.where(block, refs, cells["glyph"])
    cells["fg"] = rng.choice(colours, (rows, cols))
    cells["bg"] = rng.choice(colours, (rows, cols))
    repeat = rng.random((rows, cols)) < 0.5  # repeated colour pairs: no second escape
    for y in range(rows):
        for x in range(1, cols):
            if repeat[y, x]:
                cells["fg"][y, x], cells["bg"][y, x] = cells["fg"][y, x - 1], cells["bg"][y, x - 1]
    return cells


@pytest.mark.parametrize("shape", [(5, 7), (1, 1)])
@pytest.mark.parametrize("in_rect", [False, True])
def test_ansi_matches_the_restatement(shape, in_rect):
    rng = np.random.default_rng(shape[1] * 2 + in_rect)
    seen_kind0 = seen_unfit = seen_fit_wide = False
    for trial in range(40):
        cells = random_cells(rng, *shape)
        if trial == 0 and shape == (5, 7):  # wide names at the row end: one that fits exactly, one that does not
            cells["glyph"][0, 5] = ref.GLYPH_BLOCK | 2
            cells["glyph"][1, 6] = ref.GLYPH_BLOCK | 2
            cells["glyph"][2, 4] = ref.GLYPH_BLOCK | 3
            cells["glyph"][2, :4] = 0x20
        for names, widths in [(NAMES, WIDTHS), (None, None), ((None, NAMES[1]), (None, None))]:
            origin = (3, 11) if in_rect else (0, 0)
            want = ref.ansi(cells, names, widths, in_rect, origin)
            got = abi.cells_ansi(cells, names, widths, in_rect, origin)
            assert got == want, (trial, names is None)
            seen_kind0 |= bool(((cells["fg"] >> 24) == 0).any())
        seen_fit_wide |= "漢".encode() in ref.ansi(cells, NAMES, WIDTHS, in_rect)
        seen_unfit |= bool((cells["glyph"][:, -1] == (ref.GLYPH_BLOCK | 2)).any())
    assert seen_kind0 and (shape == (1, 1) or (seen_unfit and seen_fit_wide))


def test_ansi_format_by_hand():
    """The byte format DESIGN.md 4.22 writes out, on a grid small enough to read."""
    cells = np.zeros((1, 4), ref.CELL_DTYPE)
    cells[0, 0] = (0x2584, (3 << 24) | 196, (4 << 24) | 0x0A141E)
    cells[0, 1] = (0x2584, (3 << 24) | 196, (4 << 24) | 0x0A141E)   # the same pair: no escape
    cells[0, 2] = (ref.GLYPH_BLOCK | 1, ref.BLACK, ref.RESET)
    cells[0, 3] = (ord("X"), 0, 0)                                   # no colour at all: nothing is emitted
    names = (["a", "é"], None)
    assert abi.cells_ansi(cells, names) == (b"\x1b[?25l\x1b[0m" b"\x1b[38;5;196;48;2;10;20;30m" + "▄▄".encode() + b"\x1b[38;5;0;49m" + "é".encode()
                                            + b"X" b"\x1b[0m\r\n" b"\x1b[0m")
    assert abi.cells_ansi(cells, names, in_rect=True, origin=(2, 5)).startswith(b"\x1b[?25l\x1b[0m\x1b[6;3H\x1b[38;5;196;")
    assert abi.cells_ansi(np.zeros((0, 0), ref.CELL_DTYPE)) == b"\x1b[?25l\x1b[0m\x1b[0m"


def test_ansi_capacity_rule():
    lib = abi.load()
    cells = random_cells(np.random.default_rng(1), 5, 7)
    want = ref.ansi(cells)
    length = C.c_uint64()
    for capacity in (0, 1, len(want) - 1, len(want), len(want) + 9):
        buf = np.full(len(want) + 32, 0xA5, np.uint8)  # canary bytes
        rc = lib.aic_cells_ansi(cells.ctypes.data, 7, 5, None, 0, buf.ctypes.data, capacity, C.byref(length))
        assert length.value == len(want)
        if capacity < len(want):
            assert rc == 1 and (buf == 0xA5).all()  # too small: AIC_ERR_INVALID and nothing written
        else:
            assert rc == 0 and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()
    assert lib.aic_cells_ansi(cells.ctypes.data, 7, 5, None, 2, None, 0, C.byref(length)) == 1  # an unknown flag
    assert lib.aic_cells_ansi(None, 7, 5, None, 0, None, 0, C.byref(length)) == 1
    assert lib.aic_cells_ansi(cells.ctypes.data, 7, 5, None, 0, None, 0, None) == 1


@pytest.mark.parametrize("characters, colors", MODE_PAIRS)
def test_edge_images_take_every_branch(characters, colors):
    """The edge images (used again on the GPU) move every counter the mode pair can move, in both checkerboard parities for Split; Braille shows all 256
    dot patterns."""
    total = dict.fromkeys(ref.COUNTERS, 0)
    glyphs = set()
    parities = set()
    for image, aux in ref.edge_images(characters):
        cells, n = ref.cells(image, aux, 7, 5, characters, colors, **ref.EDGE_POST)
        for k, v in n.items():
            total[k] += v
        glyphs |= set(cells["glyph"].ravel().tolist())
        if (characters, colors) == (ref.SPLIT, ref.COLOR_NONE):
            for x in range(7):
                parities |= {(x % 2, g) for g in cells["glyph"][:, x].tolist() if g in (0x2588, 0x2580, 0x2584)}
    want = ref.expected_counters(characters, colors)
    assert all(total[k] > 0 for k in want), total
    assert all(total[k] == 0 for k in ref.COUNTERS if k not in want), total
    if characters == ref.BRAILLE:
        assert {0x2800 + i for i in range(256)} <= glyphs
    if characters == ref.SHADES:
        assert {0x20, 0x2591, 0x2592, 0x2593, 0x2588} <= glyphs
    if (characters, colors) == (ref.SHAPES, ref.COLOR_NONE):
        assert {0x2581, 0x2584, 0x2587, 0x2594, 0x2598, 0x2580, 0x259B} <= glyphs, sorted(hex(g) for g in glyphs)
    if (characters, colors) == (ref.SPLIT, ref.COLOR_NONE):
        assert len(parities) == 6, parities
        assert any(g & ref.GLYPH_BLOCK for g in glyphs) and ord("X") in glyphs and ord(".") in glyphs
    if colors == ref.COLOR_256 and characters not in (ref.SHADES, ref.BRAILLE):  # (Braille's hue has luminance 0.75: never the ramp's ends)
        ansi = set()
        for image, aux in ref.edge_images(characters):
            cells, _ = ref.cells(image, aux, 7, 5, characters, colors, **ref.EDGE_POST)
            for plane in ("fg", "bg"):
                ansi |= {int(v) & 0xFF for v in cells[plane].ravel().tolist() if int(v) >> 24 == 3}
        assert {16, 231} <= ansi and any(232 <= a <= 255 for a in ansi) and any(17 <= a <= 230 for a in ansi)


# --- the kernel's own rule, compiled for the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """all_is_cubes_amd/csrc/aic_cells_rule.h -- the source the cells kernel inlines -- behind tests/native/cells_rule_shim.cpp, with the kernel's
    floating-point contract, and the exact sRGB8 encoder's bucket table built from the oracle's thresholds."""
    import subprocess
    from pathlib import Path

    from tests import bloom_ref

    root = Path(__file__).resolve().parents[1]
    out = tmp_path_factory.mktemp("cells_rule") / "libcells_rule_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-I", str(root / "all_is_cubes_amd" / "csrc"),
                    "-o", str(out), str(root / "tests" / "native" / "cells_rule_shim.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.shim_srgb_bucket_words.restype = C.c_uint32
    table = np.zeros(lib.shim_srgb_bucket_words(), np.uint32)
    thr = np.ascontiguousarray(bloom_ref.srgb_thresholds(), np.float32)
    assert lib.shim_srgb_buckets(C.c_void_p(thr.ctypes.data), C.c_void_p(table.ctypes.data)) == 1
    lib.shim_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                               C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    lib.shim_cells.restype = None

    def run(image, aux, cols, rows, characters, colors, exposure=1.0, tone_mapping=0, maximum_intensity=np.inf, postprocessed=False):
        (w, h), _ = ref.geometry(cols, rows, characters)
        f16 = image.dtype.itemsize == 2
        image = np.ascontiguousarray(image)
        aux = None if aux is None else np.ascontiguousarray(aux, abi.PIXEL_AUX_DTYPE)
        assert image.shape == (h, w, 4)
        cells = np.zeros((max(rows, 1), max(cols, 1)), ref.CELL_DTYPE)
        counts = np.zeros(len(ref.COUNTERS), np.uint32)
        lib.shim_cells(image.ctypes.data, None if aux is None else aux.ctypes.data, table.ctypes.data, max(cols, 1), max(rows, 1), w, characters, colors,
                       int(f16), int(postprocessed), exposure, tone_mapping, maximum_intensity, cells.ctypes.data, counts.ctypes.data)
        return cells, dict(zip(ref.COUNTERS, counts.tolist()))

    return run


@pytest.mark.parametrize("characters, colors", MODE_PAIRS)
def test_the_kernels_rule_on_the_host_equals_the_restatement(rule, characters, colors):
    """Cell for cell, all three words and the counters: the edge images as f32 and as f16, with and without records, under Clamp, Reinhard and no tone
    map, and already post-processed."""
    for k, (image, aux) in enumerate(ref.edge_images(characters)):
        posts = [ref.EDGE_POST] if k else [ref.EDGE_POST, dict(exposure=1.7, tone_mapping=1, maximum_intensity=1.5), dict(exposure=0.3), dict(postprocessed=True)]
        for post in posts:
            for img in (image, np.ascontiguousarray(image.astype(np.float16))):
                for records in ((aux,) if characters == ref.NAMES else (aux, None)):
                    want, counters = ref.cells(img.astype(np.float32), records, 7, 5, characters, colors, **post)
                    got, n = rule(img, records, 7, 5, characters, colors, **post)
                    for word in ("glyph", "fg", "bg"):
                        assert (got[word] == want[word]).all(), (k, post, img.dtype, word, got[word][got[word] != want[word]][:3], want[word][got[word] != want[word]][:3])
                    assert n == counters, (k, post)


def test_the_kernels_rule_on_random_images(rule):
    """Random colours up to 4 (and exact zeros), random records, odd grids, every mode pair."""
    rng = np.random.default_rng(11)
    for characters, colors in MODE_PAIRS:
        for cols, rows in ((9, 4), (1, 1), (2, 7)):
            (w, h), _ = ref.geometry(cols, rows, characters)
            image = (rng.random((h, w, 4)) ** 3 * 4).astype(np.float32)
            image[rng.random((h, w)) < 0.1] = 0.0
            gray = rng.random((h, w)) < 0.3
            image[gray, 1] = image[gray, 0]
            image[gray, 2] = image[gray, 0]
            aux = ref._edge_aux(h, w, cols + characters)
            for post in (dict(exposure=1.0, tone_mapping=1, maximum_intensity=2.0), dict(exposure=2.5, tone_mapping=0, maximum_intensity=1.0)):
                want, counters = ref.cells(image, aux, cols, rows, characters, colors, **post)
                got, n = rule(image, aux, cols, rows, characters, colors, **post)
                assert (got == want).all() and n == counters, (characters, colors, cols, rows, post)


def test_the_context_free_half_under_the_sanitizers(tmp_path):
    """aic_cells_host.cpp built with -DAIC_CELLS_HOST_ONLY (no HIP) into tests/native/cells_ansi_check.cpp's stand-alone program with
    -fsanitize=address,undefined: random grids at every capacity around the length needed, each buffer exactly as long as its capacity."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    exe = tmp_path / "cells_ansi_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DAIC_CELLS_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), str(root / "tests" / "native" / "cells_ansi_check.cpp"), str(root / "all_is_cubes_amd" / "csrc" / "aic_cells_host.cpp")],
                   check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "cells_ansi_check ok" in run.stdout, run.stderr[-2000:]
