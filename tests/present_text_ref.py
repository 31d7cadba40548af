"""NumPy restatement of the info text of a presentation (aic_present_split_text), for the tests.

The interactive renderer's frame-rate and statistics overlay is part of its last shader (all-is-cubes-gpu shaders/postprocess.wgsl:160-276): a texture of
character codes, one texel a character cell, and a font atlas of 16 x 16 cells with premultiplied alpha. Every output pixel looks at the four cells
nearest to it -- a glyph's outline overlaps the neighbouring cells --, takes the component-wise maximum of their atlas texels and blends
tone_mapped * (1 - text.a) + text. character_texture_size (text.rs:20-52), PostprocessUniforms::new (postprocess.rs:316-331) and
render_text_to_character_texture (text.rs:56-73) make the grid, its transform and its contents. Every step is float32 in the order DESIGN.md writes it.
It shares no code with the library; the scene, the chain, the tone map and the encoders are tests/present_ref.py's and tests/bloom_ref.py's.
"""
from __future__ import annotations

import math

import numpy as np

from tests import bloom_ref
from tests import present_ref

F = np.float32


def cell_invalid(cell) -> bool:
    cw, ch, margin = cell
    return not (1 <= cw <= 1024 and 1 <= ch <= 1024) or 2 * margin >= min(cw, ch)


def geometry(nominal, cell, origin_px=(5.0, 5.0)):
    """(cols, rows, scale [2] f32, origin [2] f32) of a viewport of `nominal` = (width, height) nominal pixels and a font `cell` = (cell width, cell
    height, margin); None where aic_text_geometry rejects."""
    if cell_invalid(cell) or not all(math.isfinite(n) and n > 0 for n in nominal):
        return None
    logical = (cell[0] - 2 * cell[2], cell[1] - 2 * cell[2])
    n = [max(1, int(math.ceil(float(nominal[a]) / float(logical[a])))) for a in range(2)]  # f64
    if max(n) > 65535:
        return None
    scale = np.array([F(nominal[a]) / F(n[a] * logical[a]) for a in range(2)], F)
    origin = np.array([F(float(origin_px[a]) / float(nominal[a])) for a in range(2)], F)
    return n[0], n[1], scale, origin


def layout(text, cols: int, rows: int):
    """(codes [rows][cols] uint8, (used columns, used rows)) of a str, or of bytes taken as UTF-8 with every malformed byte a U+FFFD."""
    if isinstance(text, (bytes, bytearray)):
        text = _decode(bytes(text))
    codes = np.zeros((rows, cols), np.uint8)
    x = y = 0
    for ch in text:
        if ch == "\n":
            x, y = 0, y + 1
            continue
        if x < cols and y < rows:
            codes[y, x] = ord(ch) if ord(ch) <= 0xFF else ord("?")
        x += 1
    ys, xs = np.nonzero(codes)
    return codes, ((int(xs.max()) + 1, int(ys.max()) + 1) if len(xs) else (0, 0))


def _decode(raw: bytes) -> str:
    """The library's decoder: the lead byte gives the length, continuation bytes are taken as they come; a stray continuation byte or a sequence cut
    off by the end is one U+FFFD."""
    out, i = [], 0
    while i < len(raw):
        c, n = raw[i], 1
        if c >= 0xF0:
            n, c = 4, c & 0x07
        elif c >= 0xE0:
            n, c = 3, c & 0x0F
        elif c >= 0xC0:
            n, c = 2, c & 0x1F
        elif c >= 0x80:
            c = 0xFFFD
        if i + n > len(raw):
            c, n = 0xFFFD, 1
        else:
            for k in range(1, n):
                c = (c << 6) | (raw[i + k] & 0x3F)
        i += n
        out.append(chr(c) if c <= 0x10FFFF and not 0xD800 <= c <= 0xDFFF else "�")  # (anything above 0xFF becomes '?' either way)
    return "".join(out)


def _axis(n_out, origin, scale, n_cells):
    """Per output pixel along one axis: (f [n] f32 the first of its two cells, p [n] f32 the position in it, in [0.5, 1.5))."""
    u = (np.arange(n_out, dtype=F) + F(0.5)) / F(n_out)
    with np.errstate(over="ignore", invalid="ignore"):
        tc = ((u - F(origin)) * F(scale)) * F(n_cells)
        f = np.floor(tc)
        p = tc - f
    low = p < F(0.5)
    f = np.where(low, f - F(1.0), f)
    p = np.where(low, p + F(1.0), p)
    return f.astype(F), p.astype(F)


def _cell_axis(f, p, i, n_cells, size, margin):
    """One of an axis's two cells: (valid [n] bool, cell index [n], texel in the atlas cell [n])."""
    c = (f + F(i)).astype(F)
    q = (p - F(i)).astype(F)
    with np.errstate(invalid="ignore"):
        inside = (c >= F(0.0)) & (c < F(n_cells))
        ft = q * F(size - 2 * margin) + F(margin)
        ok = inside & (ft >= F(0.0)) & (ft < F(size))
    ci = np.where(ok, c, F(0.0)).astype(np.int64)
    ti = np.floor(np.where(ok, ft, F(0.0))).astype(np.int64)
    return ok, ci, ti


def text_layer(out_w: int, out_h: int, atlas, cell, codes, scale, origin):
    """text [out_h][out_w][4] f32: render_text at every output pixel's centre. atlas [16 ch][16 cw][4] uint8, codes [rows][cols] uint8."""
    cw, ch, margin = cell
    atlas = np.asarray(atlas, np.uint8)
    codes = np.asarray(codes, np.uint8)
    rows, cols = codes.shape
    assert atlas.shape == (16 * ch, 16 * cw, 4)
    fx, px = _axis(out_w, origin[0], scale[0], cols)
    fy, py = _axis(out_h, origin[1], scale[1], rows)
    text = np.zeros((out_h, out_w, 4), F)
    for j in (0, 1):
        oky, cy, ty = _cell_axis(fy, py, j, rows, ch, margin)
        for i in (0, 1):
            okx, cx, tx = _cell_axis(fx, px, i, cols, cw, margin)
            k = codes[cy[:, None], cx[None, :]].astype(np.int64)
            k = np.where(k == 0, 0x20, k)
            texel = atlas[(k // 16) * ch + ty[:, None], (k % 16) * cw + tx[None, :]].astype(F) / F(255.0)
            texel = np.where((oky[:, None] & okx[None, :])[..., None], texel, F(0.0))
            text = np.maximum(text, texel)
    return text


def composite(s, bloom, intensity, tone_mapping=0, maximum_intensity=np.inf, out_f16=False, text=None):
    """present_ref.composite with `text` [h][w][4] f32 blended in after the tone map: x = tm * (1 - text.a) + text. (alpha of the text, 0 or 1 where
    `text` is None: the image without text)"""
    if text is None:
        return present_ref.composite(s, bloom, intensity, tone_mapping, maximum_intensity, out_f16)
    h, w = s.shape[:2]
    x = s[..., :3]
    i = F(intensity)
    if i > 0:
        u, v = bloom_ref._centres(w, h)
        b = bloom_ref.sample(bloom, u, v, mirror=False)[..., :3]
        x = x * (F(1.0) - i) + b * i
    x = bloom_ref.tone_map(x.astype(F), tone_mapping, maximum_intensity)
    keep = F(1.0) - text[..., 3:4]
    x = (x * keep).astype(F) + text[..., :3]
    if out_f16:
        out = np.empty((h, w, 4), np.uint16)
        out[..., :3] = bloom_ref.f16(x).astype(np.float16).view(np.uint16)
        out[..., 3] = present_ref.ONE_F16
        return out
    return bloom_ref.encode(x, np.ones((h, w), F))
