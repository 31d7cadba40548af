"""The relit scenes shared by tests/test_stale_cubes_cpu.py and tests/test_gpu_stale_cubes.py: tests/stale_scenes.py's three lit spaces A with their
edits (B = A's light under the edited blocks), a glass variant of plaza, and for each the volume B' that the light updater arrives at from A's after the
edits -- oracle.LightSession: set_cubes (Mutation::set + modified_cube_needs_update) then evaluate(), maximum_distance 8 --, the cubes whose texel
differs between the two volumes, and the oracle's Split frames of B's blocks under either volume. Everything is computed once."""
import functools

import numpy as np

import oracle
from all_is_cubes_amd import flat
from tests import scenes
from tests import stale_cubes_ref as ref
from tests import stale_scenes as S

W, HT = S.W, S.HT
MAXIMUM_DISTANCE = 8
CASES = S.CASES + ["plaza_glass"]
OPAQUE_CASES = S.CASES  # the front test's stated domain, with antialiasing None
ANTIALIASING = S.ANTIALIASING
GLASS_CUBES = [(2, 1, 7), (3, 1, 7), (4, 1, 7), (5, 1, 7), (4, 2, 7), (1, 1, 1), (2, 1, 0), (6, 1, 2)]


def base(name: str) -> str:
    """the case of tests/stale_scenes.py whose camera and edits `name` has"""
    return "plaza" if name == "plaza_glass" else name


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(space A with its light, [(cube, block index in B)]) -- stale_scenes.case's; plaza_glass: plaza with 8 cubes of alpha 0.5, lit again"""
    sp, edits, _, _ = S.case(base(name))
    if name != "plaza_glass":
        return sp, edits
    g = flat.FlatSpace(sp.lo, sp.size, blocks=list(sp.blocks), sky_kind=sp.sky_kind, sky=sp.sky.copy(), block_index=sp.block_index.copy(), light=sp.light.copy())
    glass = g.add_block(flat.atom((0.2, 0.4, 0.9, 0.5)))
    for cube in GLASS_CUBES:
        g.set(cube, glass)
    scenes._unlit(g)
    oracle.evaluate_light(g, maximum_distance=MAXIMUM_DISTANCE)
    g.block_index.setflags(write=False)
    g.light.setflags(write=False)
    return g, edits


def with_light(sp, block_index, light) -> flat.FlatSpace:
    return flat.FlatSpace(sp.lo, sp.size, blocks=sp.blocks, sky_kind=sp.sky_kind, sky=sp.sky.copy(), block_index=np.array(block_index), light=np.array(light))


@functools.lru_cache(maxsize=None)
def edited(name: str) -> flat.FlatSpace:
    """B: A's light volume under the edited blocks"""
    sp, edits = case(name)
    b = with_light(sp, sp.block_index, sp.light)
    for cube, index in edits:
        b.set(cube, index)
    return b


@functools.lru_cache(maxsize=None)
def relit(name: str):
    """(B': B's blocks under the updater's volume, the light cubes that differ from A's volume as xyz [n, 3] int32 ascending in the volume's cube
    index, the updates it took)"""
    sp, edits = case(name)
    with oracle.LightSession(sp, MAXIMUM_DISTANCE) as s:
        s.set_cubes([cube for cube, _ in edits], [index for _, index in edits])
        updates, _, left = s.evaluate()
        light = s.light()
    assert left == 0
    differ = (light != np.asarray(sp.light)).any(-1)  # [x][y][z]: argwhere's order is the cube index's
    cubes = (np.argwhere(differ) + np.asarray(sp.lo)).astype(np.int32)
    cubes.setflags(write=False)
    return with_light(sp, edited(name).block_index, light), cubes, updates


def boxes(name: str) -> np.ndarray:
    return S.boxes(base(name))


def split_of(space: flat.FlatSpace, name: str, antialiasing: int):
    """(colour [HT, W, 4] uint16 f16 bit patterns, depth [HT, W] float32) of `space` under the case's camera: stale_scenes.oracle_split for any space"""
    osp = oracle.Space(space)
    inv, _, zw = S.camera(base(name))
    opt = S.options(antialiasing)
    points = S.SAMPLE_POINTS if antialiasing == 2 else [(0.5, 0.5)]
    color = np.zeros((HT, W, 4), np.float32)
    depth = np.zeros((HT, W), np.float64)
    for y in range(HT):
        y0, y1 = -(y / HT * 2.0 - 1.0), -((y + 1) / HT * 2.0 - 1.0)
        for x in range(W):
            x0, x1 = x / W * 2.0 - 1.0, (x + 1) / W * 2.0 - 1.0
            total, d = np.zeros(4, np.float32), np.inf
            for ux, uy in points:
                px, py = (x0 + (x1 - x0) * ux, y0 + (y1 - y0) * uy) if len(points) == 4 else ((x0 + x1) / 2.0, (y0 + y1) / 2.0)
                _, cb, ds = oracle.trace_ray(osp, opt, *oracle.project_ndc_into_world(inv, px, py), include_sky=True)
                total = total + cb  # f32, in sample order
                d = min(d, ds)
            cb = total / np.float32(4.0) if len(points) == 4 else total
            color[y, x, :3] = cb[:3]
            color[y, x, 3] = np.clip(np.float32(1.0) - cb[3], np.float32(0.0), np.float32(1.0))
            depth[y, x] = d
    with np.errstate(over="ignore"):
        bits = color.astype(np.float16).view(np.uint16)
    t = np.clip(depth, 0.0, 1.0)
    value = (((0.0 * 0.0 + 0.0 * 0.0) + t * zw[0]) + zw[1]) / (((0.0 * 0.0 + 0.0 * 0.0) + t * zw[2]) + zw[3])
    out = (bits, value.astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frame(name: str, which: str, antialiasing: int):
    """which = "A" | "B" (A's light) | "B'" (the updater's light)"""
    if name != "plaza_glass" and which in ("A", "B"):
        return S.oracle_split(name, which, antialiasing)
    return split_of({"A": lambda: case(name)[0], "B": lambda: edited(name), "B'": lambda: relit(name)[0]}[which](), name, antialiasing)


@functools.lru_cache(maxsize=None)
def stale_set(name: str, antialiasing: int, flags: int, with_boxes: bool = False):
    """(S [HT * W] bool, the rectangles) from tests/stale_cubes_ref.py: the relight's light cubes (with_boxes: and the edits' boxes, expand = 1), under
    the resident frame a depth flag reads -- B under A's light, or A itself when the edits are still to be traced too"""
    _, vp, _ = S.camera(base(name))
    b = boxes(name) if with_boxes else np.zeros((0, 6), np.int32)
    r = ref.rects(vp, W, HT, b, relit(name)[1], 1)
    bits, depth = frame(name, "A" if with_boxes else "B", antialiasing) if flags else (None, None)
    s = ref.stale_mask(W, HT, r, len(b), bits, depth, flags)
    s.setflags(write=False)
    r.setflags(write=False)
    return s, r
