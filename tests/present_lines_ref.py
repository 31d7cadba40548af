"""NumPy restatement of the line pass of a presentation (aic_present_split_lines), for the tests.

A line list -- pairs of world-space vertices with a linear RGBA colour -- drawn into the scene texture S of tests/present_ref.py before the bloom chain
and the composite read it, depth-tested against the resident Split frame's depth plane: where the reference draws its cursor and debug lines
(all-is-cubes-gpu everything.rs:616-658, shaders/blocks-and-lines.wgsl:902-919, pipelines.rs:453-487, the depth of shaders/rt-copy.wgsl:55-71). WebGPU
leaves line rasterisation to the implementation, so the rule is DESIGN's own, written here as DESIGN writes it: every step float32, one rounding per
operation, in the order stated. Fragments are found by testing every pixel centre of the major axis against [p0, p1), not by the index arithmetic the
kernel uses.
"""
from __future__ import annotations

import numpy as np

from tests import bloom_ref
from tests import present_ref

F = np.float32
COUNTS = ("n_clipped_away", "n_fragments", "n_passed", "n_pixels")


def segment(va, vb, m, width: int, height: int):
    """Rules 1-3 and the ordering of rule 4 for one line; va, vb = [7] (position, colour), m = [16] column-major. None: the line is dropped. Else a dict:
    x_major; p, q, d = (start, end) of the major and minor screen coordinate and the depth; c = ([3], [3]) the colours; the major coordinate ascends."""
    a, b, m = np.asarray(va, F), np.asarray(vb, F), np.asarray(m, F)
    with np.errstate(all="ignore"):
        if not (np.isfinite(a[:6]).all() and np.isfinite(b[:6]).all()):  # position and r, g, b: alpha is never read
            return None
        # 1: clip coordinates
        ca = [((m[r] * a[0] + m[4 + r] * a[1]) + m[8 + r] * a[2]) + m[12 + r] for r in range(4)]
        cb = [((m[r] * b[0] + m[4 + r] * b[1]) + m[8 + r] * b[2]) + m[12 + r] for r in range(4)]
        if not (np.isfinite(ca).all() and np.isfinite(cb).all()):
            return None
        # 2: Liang-Barsky against w + x, w - x, w + y, w - y, z, w - z
        def bounds(c):
            return [c[3] + c[0], c[3] - c[0], c[3] + c[1], c[3] - c[1], c[2], c[3] - c[2]]
        t_in, t_out, clipped_in, clipped_out = F(0.0), F(1.0), False, False
        for fa, fb in zip(bounds(ca), bounds(cb)):
            na, nb = fa < 0, fb < 0
            if na and nb:
                return None
            if na or nb:
                t = fa / (fa - fb)
                if not np.isfinite(t):
                    return None
                if na:
                    clipped_in, t_in = True, max(t_in, t)
                else:
                    clipped_out, t_out = True, min(t_out, t)
        if t_in > t_out:
            return None
        e, g = ca + [a[3], a[4], a[5]], cb + [b[3], b[4], b[5]]  # clip x, y, z, w, then r, g, b: alpha is not used
        ea = [x + t_in * (y - x) for x, y in zip(e, g)] if clipped_in else e
        eb = [x + t_out * (y - x) for x, y in zip(e, g)] if clipped_out else g
        # 3: screen coordinates
        if not (ea[3] > 0 and eb[3] > 0):
            return None
        def screen(v):
            return [((v[0] / v[3]) * F(0.5) + F(0.5)) * F(width), (F(0.5) - (v[1] / v[3]) * F(0.5)) * F(height), v[2] / v[3]]
        sa, sb = screen(ea), screen(eb)
        if not np.isfinite(sa + sb + ea[4:] + eb[4:]).all():
            return None
        # 4: the major axis, its coordinate ascending
        x_major = bool(abs(sb[0] - sa[0]) >= abs(sb[1] - sa[1]))
        pi = 0 if x_major else 1
        ends = [(sa, ea), (sb, eb)]
        if sa[pi] > sb[pi]:
            ends.reverse()
        (s0, e0), (s1, e1) = ends
        return {"x_major": x_major, "p": (s0[pi], s1[pi]), "q": (s0[1 - pi], s1[1 - pi]), "d": (s0[2], s1[2]),
                "c": (np.array(e0[4:], F), np.array(e1[4:], F))}


def fragments(seg, width: int, height: int):
    """Rule 4: (x, y, f, colour [n][3] as f32 values of f16) of the line's fragments inside the window, in ascending major index."""
    n_major, n_minor = (width, height) if seg["x_major"] else (height, width)
    (p0, p1), (q0, q1), (d0, d1), (c0, c1) = seg["p"], seg["q"], seg["d"], seg["c"]
    with np.errstate(all="ignore"):
        i = np.arange(n_major)
        centre = i.astype(F) + F(0.5)
        i = i[(centre >= p0) & (centre < p1)]
        t = ((i.astype(F) + F(0.5)) - p0) / (p1 - p0)
        jf = np.floor(q0 + t * (q1 - q0))
        keep = (jf >= F(0.0)) & (jf < F(n_minor))
        i, t, j = i[keep], t[keep], jf[keep].astype(np.int64)
        f = np.fmin(np.fmax(d0 + t * (d1 - d0), F(0.0)), F(1.0))
        colour = bloom_ref.f16(c0[None, :] + t[:, None] * (c1 - c0)[None, :])
    x, y = (i, j) if seg["x_major"] else (j, i)
    return x, y, f, colour


def depth_texels(depth_bits, width: int, height: int):
    """Rule 5's texel of every output pixel [height][width] u32: the pixel's own at equal size, else the nearest by the pixel centre."""
    depth_bits = np.asarray(depth_bits, np.uint32)
    sh, sw = depth_bits.shape
    if (sw, sh) == (width, height):
        return depth_bits
    tx = np.minimum(((np.arange(width).astype(F) + F(0.5)) / F(width) * F(sw)).astype(np.uint32), sw - 1)
    ty = np.minimum(((np.arange(height).astype(F) + F(0.5)) / F(height) * F(sh)).astype(np.uint32), sh - 1)
    return depth_bits[ty[:, None], tx[None, :]]


def draw(s, depth_bits, vertices, m, stats=None):
    """S' and the counts: s = present_ref.scene's [h][w][4], depth_bits [src_h][src_w] u32, vertices [2 n][7], m [16]. `stats`, a dict, receives
    `contested`: the pixels where two passing fragments met, and `ties`: those of them where the two least depths were equal."""
    h, w = s.shape[:2]
    vertices = np.asarray(vertices, F).reshape(-1, 2, 7)
    texel_bits = depth_texels(depth_bits, w, h)
    texel = texel_bits.view(F)
    with np.errstate(invalid="ignore"):
        limit = np.where((texel_bits >> 31).astype(bool) | np.isnan(texel), F(-1.0), np.fmin(texel, F(1.0)))  # f >= 0 is never below -1
    out = np.array(s, F)
    best = np.full((h, w), np.inf)  # the winner's f (f32 values in f64: exact), then its line
    second = np.full((h, w), np.inf)
    owner = np.full((h, w), -1, np.int64)
    counts = dict.fromkeys(COUNTS, 0)
    for index, (va, vb) in enumerate(vertices):
        seg = segment(va, vb, m, w, h)
        if seg is None:
            counts["n_clipped_away"] += 1
            continue
        x, y, f, colour = fragments(seg, w, h)
        counts["n_fragments"] += len(x)
        passed = f < limit[y, x]
        x, y, f, colour = x[passed], y[passed], f[passed], colour[passed]
        counts["n_passed"] += len(x)
        second[y, x] = np.minimum(second[y, x], np.maximum(f, best[y, x]))
        wins = f < best[y, x]  # Less: an equal depth leaves the earlier line
        x, y = x[wins], y[wins]
        best[y, x] = f[wins]
        owner[y, x] = index
        out[y, x, :3] = colour[wins]
        out[y, x, 3] = F(1.0)
    counts["n_pixels"] = int((owner >= 0).sum())
    if stats is not None:
        stats["contested"] = int(np.isfinite(second).sum())
        stats["ties"] = int((np.isfinite(second) & (second == best)).sum())
        stats["owner"] = owner
    return out, counts


def present(color_bits, depth_bits, out_size, vertices, m, intensity, tone_mapping=0, maximum_intensity=np.inf, out_f16=False, parts=None):
    """aic_present_split_lines: (image, counts). `parts` as present_ref.present's, with "S'" and "counts" beside S and B."""
    parts = {} if parts is None else parts
    if "S'" not in parts:
        if "S" not in parts:
            parts["S"] = present_ref.scene(color_bits, *out_size)
        parts["S'"], parts["counts"] = draw(parts["S"], depth_bits, vertices, m)
    if F(intensity) > 0 and parts.get("B'") is None:
        parts["B'"] = present_ref.chain(parts["S'"])
    return present_ref.composite(parts["S'"], parts.get("B'"), intensity, tone_mapping, maximum_intensity, out_f16), parts["counts"]
