"""NumPy / plain-Python restatement of the terminal's character cells (aic_cells_geometry, aic_image_cells, aic_render_cells, aic_cells_ansi;
DESIGN.md 4.22), for the tests.

The patch rule is image_patch_to_character (all-is-cubes-desktop/src/terminal/chars.rs:18-173) with ColorMode::convert (terminal/options.rs:78-139) on
pixels made by camera.post_process_color(Rgba::from(ColorBuf)) (terminal.rs:355-365); the byte stream is write_frame with write_colored_and_measure
(terminal/ui.rs:300-360, chars.rs:205-296). Every colour operation is float32, one rounding each, in the order the reference writes it.
"""
from __future__ import annotations

import numpy as np

from tests import bloom_ref

F = np.float32

NAMES, SHADES, SPLIT, SHAPES, BRAILLE = range(5)
COLOR_NONE, COLOR_256, COLOR_RGB = range(3)
CHARACTER_MODES = (NAMES, SHADES, SPLIT, SHAPES, BRAILLE)
COLOR_MODES = (COLOR_NONE, COLOR_256, COLOR_RGB)
RAYS = {NAMES: (1, 1), SHADES: (1, 1), SPLIT: (1, 2), SHAPES: (1, 2), BRAILLE: (2, 4)}
GLYPH_BLOCK = 0x80000000
KIND_NONE, KIND_RESET, KIND_BLACK, KIND_ANSI, KIND_RGB = range(5)
RESET, BLACK = KIND_RESET << 24, KIND_BLACK << 24

CELL_DTYPE = np.dtype([("glyph", "<u4"), ("fg", "<u4"), ("bg", "<u4")])
COUNTERS = ("n_full", "n_upper", "n_lower", "n_text", "n_space", "n_shade", "n_rising", "n_falling", "n_equal", "n_unequal", "n_names", "n_braille",
            "n_gray", "n_cube", "n_rgb")


def expected_counters(characters: int, colors: int):
    """The counters a mode pair can move at all: the arms of its own branch of the rule and of its colour conversion."""
    conv = {COLOR_NONE: (), COLOR_256: ("n_gray", "n_cube"), COLOR_RGB: ("n_rgb",)}[colors]
    if characters in (SPLIT, SHAPES):
        if colors != COLOR_NONE:
            return ("n_equal", "n_unequal") + conv
        return ("n_full", "n_upper", "n_lower", "n_text", "n_space") if characters == SPLIT else ("n_shade", "n_rising", "n_falling")
    if characters == SHADES:
        return ("n_shade",)
    return (("n_names",) if characters == NAMES else ("n_braille",)) + conv


def geometry(cols: int, rows: int, characters: int):
    """TerminalOptions::viewport_from_terminal_size (options.rs:25-38): ((width, height) of the framebuffer, (nominal width, height))."""
    c, r = max(int(cols), 1), max(int(rows), 1)
    rx, ry = RAYS[characters]
    return (c * rx, r * ry), (c * 0.5, r * 1.0)


def luminance(rgb):
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return g * F(0.7152) + (r * F(0.2126) + b * F(0.0722))


def post_process(rgb, exposure, tone_mapping, maximum_intensity):
    """Camera::post_process_color (camera_struct.rs:376-382) on [..., 3] float32."""
    return bloom_ref.tone_map(bloom_ref.ps_mul(np.asarray(rgb, F), F(exposure)).astype(F), tone_mapping, maximum_intensity).astype(F)


def srgb8(x):
    """component_to_srgb8 (color.rs:1051-1054) of float32 values: the number of thresholds at or below."""
    x = np.asarray(x, F)
    thr = bloom_ref.srgb_thresholds()[1:]
    with np.errstate(invalid="ignore"):
        pos = x > 0
    return np.where(pos, np.searchsorted(thr, np.where(pos, x, F(0.0)), side="right"), 0).astype(np.int64)


def _cube_level(v):
    return (v >= 48).astype(np.int64) + (v >= 115) + (v >= 155) + (v >= 195) + (v >= 235)


def convert(colors: int, rgb, counters):
    """ColorMode::convert(Some(rgb)) as colour words; 0 under ColorMode::None."""
    rgb = np.asarray(rgb, F)
    shape = rgb.shape[:-1]
    if colors == COLOR_NONE:
        return np.zeros(shape, np.uint32)
    if colors == COLOR_256:
        lum = luminance(rgb)
        with np.errstate(invalid="ignore"):
            sat = (np.abs(rgb[..., 0] - lum) + np.abs(rgb[..., 1] - lum)) + np.abs(rgb[..., 2] - lum)
            gray_path = sat < F(0.1)
        s = srgb8(lum)
        gray = np.floor((s.astype(F) / F(255.0) * F(25.0)).astype(np.float64) + 0.5).astype(np.int64)
        gray = np.where(gray == 0, 16, np.where(gray == 25, 231, gray + 231))
        c = srgb8(rgb)
        cube = 16 + (_cube_level(c[..., 0]) * 6 + _cube_level(c[..., 1])) * 6 + _cube_level(c[..., 2])
        counters["n_gray"] += int(gray_path.sum())
        counters["n_cube"] += int((~gray_path).sum())
        return ((KIND_ANSI << 24) | np.where(gray_path, gray, cube)).astype(np.uint32)
    c = srgb8(rgb)
    counters["n_rgb"] += int(np.prod(shape))
    return ((KIND_RGB << 24) | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).astype(np.uint32)


def pixel_text(aux):
    """A pixel's glyph from its first-hit record, as HipRtRenderer::draw_text reads it; ' ' without records."""
    hit = aux["hit"] == 1
    block = GLYPH_BLOCK | ((aux["layer"].astype(np.int64) & 0x7FFF) << 16) | (aux["block_index"].astype(np.int64) & 0xFFFF)
    steps = aux["cubes_traced"]
    other = np.where(steps > 1000, ord("X"), np.where(steps > 0, ord(" "), ord(".")))
    return np.where(hit, block, other).astype(np.uint32)


def _pick_index(position, n: int):
    """pick_01_from_array's index (chars.rs:175-182): a truncating, saturating cast, then the clamp."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(position, F) * F(n)
        pos = v > 0
        return np.where(pos, np.where(v >= n, n - 1, np.trunc(np.where(pos & (v < n), v, 0))), 0).astype(np.int64)


_SHADE = np.array([0x20, 0x2591, 0x2592, 0x2593, 0x2588], np.uint32)                                          # " ░▒▓█"
_RISING = np.array([0x20, 0x2581, 0x2582, 0x2583, 0x2584, 0x2585, 0x2586, 0x2587, 0x2588], np.uint32)         # " ▁▂▃▄▅▆▇█"
_FALLING = np.array([0x20, 0x2594, 0x2598, 0x2598, 0x2580, 0x2580, 0x259B, 0x259B, 0x2588], np.uint32)        # " ▔▘▘▀▀▛▛█"
# dot k + 1 of a Braille cell is bit k: (dx, dy) in the 2 x 4 patch, dots numbered 1 4 / 2 5 / 3 6 / 7 8
_DOTS = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (0, 3), (1, 3))


def cells(image, aux, cols: int, rows: int, characters: int, colors: int, exposure=1.0, tone_mapping=0, maximum_intensity=np.inf, postprocessed=False):
    """aic_image_cells: (cells [rows][cols] of CELL_DTYPE, counters). image = [height][width][>= 3] float32 of the geometry's framebuffer; aux =
    [height][width] of abi.PIXEL_AUX_DTYPE or None."""
    (w, h), _ = geometry(cols, rows, characters)
    cols, rows = max(cols, 1), max(rows, 1)
    rgb = np.asarray(image, F)[..., :3]
    assert rgb.shape[:2] == (h, w), (rgb.shape, (h, w))
    if not postprocessed:
        rgb = post_process(rgb, exposure, tone_mapping, maximum_intensity)
    if characters == NAMES and aux is None:
        raise ValueError("Names needs the first-hit records")
    text = pixel_text(aux) if aux is not None else np.full((h, w), ord(" "), np.uint32)
    n = dict.fromkeys(COUNTERS, 0)
    out = np.zeros((rows, cols), CELL_DTYPE)
    cx = np.broadcast_to(np.arange(cols)[None, :], (rows, cols))
    cy = np.broadcast_to(np.arange(rows)[:, None], (rows, cols))
    if characters in (SPLIT, SHAPES):
        c1, c2 = rgb[0::2], rgb[1::2]
        if colors == COLOR_NONE:
            lum1, lum2 = luminance(c1), luminance(c2)
            if characters == SPLIT:
                even = cx % 2 == 0
                t1, t2 = np.where(even, F(0.5), F(0.7)), np.where(even, F(0.7), F(0.5))
                with np.errstate(invalid="ignore"):
                    up, down, fallback = lum1 > t1, lum2 > t2, lum2 > F(0.2)
                arms = {"n_full": up & down, "n_upper": up & ~down, "n_lower": ~up & down, "n_text": ~up & ~down & fallback, "n_space": ~up & ~down & ~fallback}
                glyph = np.select([arms["n_full"], arms["n_upper"], arms["n_lower"], arms["n_text"]], [np.int64(0x2588), np.int64(0x2580), np.int64(0x2584), text[0::2].astype(np.int64)], np.int64(0x20))
            else:
                avg = ((lum1.astype(np.float64) + lum2.astype(np.float64)) / 2.0).astype(F)  # f32::midpoint
                with np.errstate(invalid="ignore"):
                    avg = np.where(avg < 0, F(0.0), np.where(avg > 1, F(1.0), avg)).astype(F)
                    close, rising = np.abs(lum1 - lum2) < F(0.05), lum1 < lum2
                arms = {"n_shade": close, "n_rising": ~close & rising, "n_falling": ~close & ~rising}
                i5, i9 = _pick_index(avg, 5), _pick_index(avg, 9)
                glyph = np.select([arms["n_shade"], arms["n_rising"]], [_SHADE[i5], _RISING[i9]], _FALLING[i9])
            for k, m in arms.items():
                n[k] += int(m.sum())
            out["glyph"] = glyph
        else:
            k1, k2 = convert(colors, c1, n), convert(colors, c2, n)
            equal = k1 == k2
            n["n_equal"] += int(equal.sum())
            n["n_unequal"] += int((~equal).sum())
            out["glyph"] = np.where(equal, 0x20, 0x2584)
            out["fg"] = np.where(equal, BLACK, k2)
            out["bg"] = k1
    elif characters == NAMES:
        k = convert(colors, rgb, n)
        out["glyph"] = text
        out["fg"] = np.where(k != 0, BLACK, RESET)
        out["bg"] = np.where(k != 0, k, RESET)
        n["n_names"] += rows * cols
    elif characters == SHADES:
        out["glyph"] = _SHADE[_pick_index(luminance(rgb), 5)]
        out["fg"] = out["bg"] = RESET
        n["n_shade"] += rows * cols
    else:
        base = cx.astype(F) * F(284.1834) + cy.astype(F) * F(100.2384)
        index = np.zeros((rows, cols), np.int64)
        total = None
        for k, (dx, dy) in enumerate(_DOTS):
            c = rgb[dy::4, dx::2]
            threshold = (np.fmod(F(k) + base, F(8.0)) + F(0.5)) / F(8.0)
            with np.errstate(invalid="ignore"):
                index |= (luminance(c) > threshold).astype(np.int64) << k
            total = c if total is None else total + c
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = F(0.75) / np.fmax(luminance(total), F(0.1))
            scale = np.where(scale > 0, scale, F(0.0)).astype(F)
        k_ = convert(colors, bloom_ref.ps_mul(total, scale[..., None]).astype(F), n)
        out["glyph"] = 0x2800 + index
        out["fg"] = np.where(k_ != 0, k_, RESET)
        out["bg"] = np.where(k_ != 0, BLACK, RESET)
        n["n_braille"] += rows * cols
    return out, n


def glyph_text(cells_row) -> str:
    """A row of cells as a string, block references as '*' (what the reference's own tests of the rule fill in)."""
    return "".join("*" if g & GLYPH_BLOCK else chr(g) for g in cells_row["glyph"].tolist())


# --- the byte stream -------------------------------------------------------------------------------------------------------------------------------------
def _sgr(word: int, foreground: bool):
    kind, payload = word >> 24, word & 0xFFFFFF
    lead = "38" if foreground else "48"
    if kind == KIND_RESET:
        return "39" if foreground else "49"
    if kind == KIND_BLACK:
        return f"{lead};5;0"
    if kind == KIND_ANSI:
        return f"{lead};5;{payload & 0xFF}"
    if kind == KIND_RGB:
        return f"{lead};2;{(payload >> 16) & 0xFF};{(payload >> 8) & 0xFF};{payload & 0xFF}"
    return None


def ansi(cells_, names=None, widths=None, in_rect: bool = False, origin=(0, 0)) -> bytes:
    """aic_cells_ansi. names / widths: per layer (world, ui) a list of str / int, or None."""
    names = names or (None, None)
    widths = widths or (None, None)
    rows, cols = cells_.shape
    out = [b"\x1b[?25l", b"\x1b[0m"]
    current = None
    for y in range(rows):
        if in_rect:
            out.append(f"\x1b[{origin[1] + y + 1};{origin[0] + 1}H".encode())
        x = 0
        while x < cols:
            glyph, fg, bg = (int(v) for v in cells_[y, x])
            if current != (fg, bg):
                current = (fg, bg)
                parts = [s for s in (_sgr(fg, True), _sgr(bg, False)) if s is not None]
                if parts:
                    out.append(("\x1b[" + ";".join(parts) + "m").encode())
            width = 1
            if glyph & GLYPH_BLOCK:
                layer, index = (glyph >> 16) & 0x7FFF, glyph & 0xFFFF
                table = names[layer] if layer < 2 else None
                if table is not None and index < len(table) and table[index] is not None:
                    text = table[index].encode()
                    if widths[layer] is not None:
                        width = int(widths[layer][index])
                else:
                    text = b"#"
            else:
                text = ("�" if 0xD800 <= glyph <= 0xDFFF or glyph > 0x10FFFF else chr(glyph)).encode()
            if width <= cols - x:
                out.append(text)
            x += max(width, 1)
        if not in_rect:
            current = None
            out.append(b"\x1b[0m\r\n")
    out.append(b"\x1b[0m")
    return b"".join(out)


# --- inputs the CPU and the GPU tests share --------------------------------------------------------------------------------------------------------------
RAMP = (0.0, 0.9, 1.1, 1.9, 2.1, 2.9, 3.1, 3.9, 4.1, 5.0)  # chars.rs:350-404


def ramp_image(rows_of: str):
    """The images of the reference's four tests of the rule: 10 columns; rows_of = 'r' (the ramp), 'rr' (two equal rows), 'br' (black above the ramp)."""
    ramp = np.array([F(v) / F(5.0) for v in RAMP], F)
    img = np.zeros((len(rows_of), 10, 4), F)
    for y, kind in enumerate(rows_of):
        img[y, :, :3] = ramp[:, None] if kind == "r" else F(0.0)
    img[..., 3] = 1.0
    return img


# the post-processing the edge images are made for: targets t are stored as t / 0.5 (exact), and whatever lies above 2 after exposure is clamped
EDGE_POST = dict(exposure=0.5, tone_mapping=0, maximum_intensity=2.0)


def _around(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def edge_pool():
    """Post-processed target colours at and next to every threshold of the rule."""
    thr = bloom_ref.srgb_thresholds()
    grays = [F(0.0), F(1.0), F(1.5), F(3.0)]  # (above 1; above the tone map's maximum: clamped)
    for v in (0.05, 0.1, 0.2, 0.5, 0.7, 0.3, 0.6, 0.9):
        grays += _around(v)
    for s in (5, 6, 15, 16, 117, 118, 127, 128, 239, 240, 249, 250, 255):  # the grey ramp's halves: s / 255 * 25 next to k + 0.5; both ends
        grays += [thr[s], np.nextafter(thr[s], F(0.0))]
    pool = [(g, g, g) for g in grays]
    for d in (0.0824, 0.082467, 0.0825, 0.0826):  # saturation 1.2126 d at and next to 0.1
        for v in _around(d):
            pool.append((F(0.5) + v, F(0.5), F(0.5)))
    for k in (48, 115, 155, 195, 235):  # the colour cube's breaks, in every channel, beside a channel that keeps the colour saturated
        for t in (thr[k], np.nextafter(thr[k], F(0.0))):
            pool += [(t, F(1.0), F(0.0)), (F(0.0), t, F(1.0)), (F(1.0), F(0.0), t)]
    pool += [(F(1.0), F(0.0), F(0.0)), (F(0.0), F(1.0), F(0.0)), (F(0.0), F(0.0), F(1.0)), (F(2.0), F(0.25), F(0.0)), (F(0.9), F(0.8), F(0.1))]
    return np.array(pool, F)


def _edge_aux(h: int, w: int, seed: int):
    from all_is_cubes_amd import abi

    rng = np.random.default_rng(seed)
    aux = np.zeros((h, w), abi.PIXEL_AUX_DTYPE)
    aux["hit"] = rng.integers(0, 2, (h, w))
    aux["block_index"] = rng.integers(0, 9, (h, w))
    aux["layer"] = rng.integers(0, 2, (h, w))
    aux["cubes_traced"] = rng.choice(np.array([0, 1, 1000, 1001, 5000], np.uint32), (h, w))
    return aux


def edge_images(characters: int, cols: int = 7, rows: int = 5):
    """[(image [h][w][4] float32, aux [h][w])]: the pool laid over as many cols x rows grids as it takes -- every pixel of a 1 x 1 mode, upper / lower pairs
    both equal and unequal of a 1 x 2 mode, and for Braille every one of the 256 dot patterns (white and black dots) and the pool as cell colours."""
    pool = edge_pool() / F(EDGE_POST["exposure"])
    (w, h), _ = geometry(cols, rows, characters)
    n_cells = cols * rows
    rx, ry = RAYS[characters]
    per_cell = []  # [ry][rx][3] patches
    if characters in (NAMES, SHADES):
        per_cell = [c.reshape(1, 1, 3) for c in pool]
    elif characters in (SPLIT, SHAPES):
        p = len(pool)
        for i in range(p):
            per_cell.append(np.stack([pool[i], pool[(i * 7 + 3) % p]]).reshape(2, 1, 3))
            per_cell.append(np.stack([pool[(i * 5 + 1) % p], pool[i]]).reshape(2, 1, 3))
            if i % 3 == 0:
                per_cell.append(np.stack([pool[i], pool[i]]).reshape(2, 1, 3))
    else:
        for index in range(256):
            patch = np.zeros((4, 2, 3), F)
            for k, (dx, dy) in enumerate(_DOTS):
                patch[dy, dx] = F(4.0) if index >> k & 1 else F(0.0)  # (a dot's threshold reaches 1.0625)
            per_cell.append(patch)
        for c in pool:
            per_cell.append(np.broadcast_to(c / F(8.0), (4, 2, 3)).copy())
    images = []
    for first in range(0, len(per_cell), n_cells):
        img = np.zeros((h, w, 4), F)
        img[..., 3] = 1.0
        for j in range(n_cells):
            patch = per_cell[(first + j) % len(per_cell)]
            y, x = divmod(j, cols)
            img[y * ry:(y + 1) * ry, x * rx:(x + 1) * rx, :3] = patch
        images.append((img, _edge_aux(h, w, len(images) + 17 * characters)))
    return images
