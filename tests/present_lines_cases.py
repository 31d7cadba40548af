"""The frames and line lists the tests of aic_present_split_lines share (tests/test_present_lines_cpu.py checks from the restatement alone that they
test something; tests/test_gpu_present_lines.py runs them on the device). Everything is seeded and depends on the sizes and the count only."""
from __future__ import annotations

import functools

import numpy as np

from tests import present_lines_ref as ref
from tests import present_ref, reproject_ref

F = np.float32
SIZES = [((1, 1), (1, 1)), ((3, 5), (3, 5)), ((17, 9), (17, 9)), ((64, 48), (64, 48)), ((32, 24), (64, 48)), ((64, 48), (17, 9)), ((257, 129), (257, 129))]
N_LINES = [1, 28, 65, 1000]
NEAR, FAR = 1.0, 10.0
MARKER = (0, 0, 0, 0xBC00)


def synthetic_frame(w, h):
    """(colour [h, w, 4] u16, depth [h, w] u32 bit patterns). Colours as tests/test_gpu_present.py makes them: exponential-random f16 >= 0, some infinity
    or 65504, marker texels. Depth: values in (0, 1) mostly; a tenth exactly 1.0; then a twentieth each above 1 (infinity among them), -0.0, negative
    and NaN. Texel (0, 0) is 0.75: a window of one pixel can show a line."""
    rng = np.random.default_rng(3000 * w + h)
    color = rng.exponential(2.0, (h, w, 4)).astype(np.float16).view(np.uint16)
    color[..., 3] = rng.random((h, w)).astype(np.float16).view(np.uint16)
    top = rng.random((h, w, 3)) < 0.01
    color[..., :3][top] = np.where(rng.random(int(top.sum())) < 0.5, 0x7C00, 0x7BFF).astype(np.uint16)
    if w * h >= 4:
        color[rng.random((h, w)) < 0.05] = MARKER
    depth = (F(0.05) + F(0.95) * rng.random((h, w)).astype(F)).astype(F)
    kind = rng.random((h, w))
    depth[kind < 0.10] = 1.0
    depth[(kind >= 0.10) & (kind < 0.15)] = np.where(rng.random(int(((kind >= 0.10) & (kind < 0.15)).sum())) < 0.5, np.inf, 1.5).astype(F)
    depth[(kind >= 0.15) & (kind < 0.20)] = -0.0
    depth[(kind >= 0.20) & (kind < 0.25)] = -0.25
    depth[(kind >= 0.25) & (kind < 0.30)] = np.nan
    depth[0, 0] = 0.75
    return color, depth.view(np.uint32)


def view_projection(w, h):
    """[16] f32 column-major: a 90-degree perspective of the window's aspect, near 1, far 10, seen from the origin down -z with a little yaw."""
    pv = reproject_ref.perspective(90.0, w / h, NEAR, FAR) @ reproject_ref.view(yaw=0.05, position=(0.1, -0.05, 0.0))
    return pv.T.reshape(16).astype(F)


def _world(m, w, h, sx, sy, dist):
    """the world point that the matrix sends to window position (sx, sy) at eye distance `dist` (clip w)"""
    pv = np.asarray(m, np.float64).reshape(4, 4).T
    z_clip = FAR / (NEAR - FAR) * -dist + NEAR * FAR / (NEAR - FAR)
    clip = np.array([(sx / w * 2.0 - 1.0) * dist, (1.0 - sy / h * 2.0) * dist, z_clip, dist])
    p = np.linalg.solve(pv, clip)
    return p[:3] / p[3]


def line_list(n, w, h):
    """[2 n][7] f32: random in-view segments, segments with one end behind the camera, wholly outside, of zero length, axis-aligned, exactly diagonal,
    with endpoints on pixel centres, duplicates of earlier lines, two-coloured; from 28 lines on, one vertex has a NaN. One line alone crosses the whole
    window."""
    rng = np.random.default_rng(7919 * n + 100 * w + h)
    m = view_projection(w, h)
    v = np.zeros((n, 2, 7), F)
    v[..., 6] = 1.0
    def anywhere():
        return _world(m, w, h, rng.uniform(-0.1 * w, 1.1 * w), rng.uniform(-0.1 * h, 1.1 * h), rng.uniform(1.1, 9.5))
    for k in range(n):
        kind = k % 10
        colour = rng.uniform(0.0, 4.0, 3)
        v[k, :, 3:6] = colour
        if n == 1:
            a, b = _world(m, w, h, -0.5, 0.1 * h, 1.2), _world(m, w, h, w + 0.5, 0.9 * h, 9.0)
        elif kind in (0, 9):
            a, b = anywhere(), anywhere()
        elif kind == 1:  # one end behind the camera
            a, b = anywhere(), _world(m, w, h, rng.uniform(0, w), rng.uniform(0, h), -rng.uniform(0.5, 3.0))
        elif kind == 2:  # wholly outside: to the right of the window, or beyond the far plane
            a, b = ((_world(m, w, h, 1.5 * w, 0.2 * h, 3.0), _world(m, w, h, 2.5 * w, 0.8 * h, 5.0)) if k % 20 == 2 else
                    (_world(m, w, h, 0.3 * w, 0.3 * h, 11.0), _world(m, w, h, 0.6 * w, 0.6 * h, 15.0)))
        elif kind == 3:  # zero length
            a = anywhere()
            b = a
        elif kind == 4:  # axis-aligned on the screen, at one distance
            dist, x0, y0 = rng.uniform(1.5, 8.0), int(rng.integers(0, w)), int(rng.integers(0, h))
            a = _world(m, w, h, x0 + 0.25, y0 + 0.5, dist)
            b = _world(m, w, h, w - 0.25, y0 + 0.5, dist) if k % 20 == 4 else _world(m, w, h, x0 + 0.25, h + 2.0, dist)
        elif kind == 5:  # exactly diagonal: |dx| = |dy|
            dist, span = rng.uniform(1.5, 8.0), min(w, h)
            a, b = _world(m, w, h, 0.0, 0.0, dist), _world(m, w, h, float(span), float(span), dist * 1.5)
        elif kind == 6:  # endpoints on pixel centres
            x0, y0, x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(0, h))
            a, b = _world(m, w, h, x0 + 0.5, y0 + 0.5, rng.uniform(1.2, 9.0)), _world(m, w, h, x1 + 0.5, y1 + 0.5, rng.uniform(1.2, 9.0))
        elif kind == 7:  # a line drawn twice, the second time in another colour: equal depths, the earlier one shows
            a, b = v[k - 7, 0, :3], v[k - 7, 1, :3]
        else:  # two colours
            a, b = anywhere(), anywhere()
            v[k, 1, 3:6] = rng.uniform(0.0, 4.0, 3)
        v[k, 0, :3], v[k, 1, :3] = a, b
    if n >= 28:
        v[12, 1, 1] = np.nan
    return v.reshape(2 * n, 7)


@functools.lru_cache(maxsize=None)
def restated(src, out, n):
    """(colour, depth, vertices, m, parts, stats): the frame, the list, and what of the restatement does not depend on the presentation's options --
    S, S', the counts, B of S' -- with the draw's statistics."""
    color, depth = synthetic_frame(*src)
    vertices, m = line_list(n, *out), view_projection(*out)
    parts, stats = {"S": present_ref.scene(color, *out)}, {}
    parts["S'"], parts["counts"] = ref.draw(parts["S"], depth, vertices, m, stats)
    for a in (color, depth, vertices, m, parts["S"], parts["S'"]):
        a.setflags(write=False)
    return color, depth, vertices, m, parts, stats


def bloom_of(parts):
    """B of S', computed once per case and kept in `parts`"""
    if parts.get("B'") is None:
        parts["B'"] = present_ref.chain(parts["S'"])
        parts["B'"].setflags(write=False)
    return parts["B'"]
