"""The scene edits shared by tests/test_stale_cpu.py and tests/test_gpu_stale.py: small lit spaces A, the same spaces B after a few cubes changed under an
UNCHANGED light volume, the boxes of those cubes, a camera, and the oracle's Split frame of either -- raytrace_to_texture.rs:623-675 on oracle.trace_ray's
ColorBuf and DepthBuf of every sample ray, as tests/test_gpu_split.py composes it, for a world layer alone and exposure 1. Everything is computed once."""
import functools

import numpy as np

import oracle
from all_is_cubes_amd import _host as H
from all_is_cubes_amd import flat
from tests import scenes, stale_ref

W, HT = 96, 64
VIEW_DISTANCE = 200.0
SAMPLE_POINTS = [(1 / 8, 5 / 8), (3 / 8, 1 / 8), (5 / 8, 7 / 8), (7 / 8, 3 / 8)]  # renderer.rs:428-433
CASES = ["plaza", "terrace", "behind_wall"]  # behind_wall: opaque only, for AIC_STALE_DEPTH_TEST
ANTIALIASING = [0, 2]  # None, Always


def _blocks(sp):
    """air, floor, red, green, a recursive block (R2 checkerboard slab), wall"""
    air = sp.add_block(flat.air())
    floor = sp.add_block(flat.atom((0.5, 0.5, 0.5, 1.0)))
    red = sp.add_block(flat.atom((0.9, 0.1, 0.1, 1.0)))
    green = sp.add_block(flat.atom((0.1, 0.8, 0.2, 1.0)))
    slab = sp.add_block(scenes.slab_block(1, 2))
    wall = sp.add_block(flat.atom((0.3, 0.3, 0.7, 1.0)))
    return air, floor, red, green, slab, wall


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(space A with its light, [(cube, block index in B)], eye, target). Every block B uses is in A's table already."""
    sp = flat.FlatSpace((0, 0, 0), (8, 4, 8))
    sp.set_sky_uniform(scenes.from_srgb8(scenes.DAY_SKY_COLOR))
    air, floor, red, green, slab, wall = _blocks(sp)
    scenes._fill(sp, (0, 0, 0), (8, 1, 8), floor)
    if name == "plaza":
        for cube, b in [((2, 1, 2), red), ((5, 1, 4), green), ((3, 1, 5), red), ((3, 2, 5), green)]:
            sp.set(cube, b)
        # a cube removed, an opaque one added beside a lit surface (the green cube's side and the floor), one swapped for a recursive block
        edits = [((2, 1, 2), air), ((4, 1, 4), red), ((3, 2, 5), slab)]
        eye, target = (4.3, 4.0, 10.0), (4.0, 1.0, 4.0)
    elif name == "terrace":
        scenes._fill(sp, (0, 1, 0), (8, 1, 3), wall)  # a step along the back
        for cube, b in [((1, 2, 1), red), ((6, 1, 5), green), ((6, 2, 1), slab)]:
            sp.set(cube, b)
        edits = [((1, 2, 1), air), ((5, 1, 5), green), ((6, 2, 1), red)]
        eye, target = (-1.0, 5.0, 9.5), (4.0, 1.0, 3.0)
    elif name == "behind_wall":
        scenes._fill(sp, (0, 1, 5), (8, 2, 1), wall)
        for cube, b in [((4, 1, 2), red), ((6, 1, 7), green)]:
            sp.set(cube, b)
        # the red cube is hidden behind the wall with everything within one cube of it; the green one stands in front
        edits = [((4, 1, 2), air), ((6, 1, 7), red)]
        eye, target = (4.0, 2.5, 11.0), (4.0, 1.5, 4.0)
    else:
        raise KeyError(name)
    scenes._unlit(sp)
    oracle.evaluate_light(sp, maximum_distance=8)
    sp.block_index.setflags(write=False)
    sp.light.setflags(write=False)
    return sp, edits, eye, target


def edited(name: str) -> flat.FlatSpace:
    """B: A's blocks and A's light volume, the edited cubes' block indices"""
    sp, edits, _, _ = case(name)
    b = flat.FlatSpace(sp.lo, sp.size, blocks=sp.blocks, sky_kind=sp.sky_kind, sky=sp.sky.copy(), block_index=sp.block_index.copy(), light=sp.light.copy())
    for cube, index in edits:
        b.set(cube, index)
    return b


def boxes(name: str) -> np.ndarray:
    """[n, 6] int32: one box of one cube per edit"""
    _, edits, _, _ = case(name)
    return np.array([[*cube, *(c + 1 for c in cube)] for cube, _ in edits], np.int32)


@functools.lru_cache(maxsize=None)
def camera(name: str):
    """(inverse projection-view for the frame, view_projection [16] f64 column-major: clip = M (x, y, z, 1), depth transform zw)"""
    _, _, eye, target = case(name)
    projection, world_to_eye, inv = oracle.camera_matrices(90.0, VIEW_DISTANCE, W / HT, oracle.look_at_y_up(eye, target), eye)
    # euclid's row-vector matrices in m11..m44 order: view.then(projection), read column-major, is the column-vector product
    vp = (world_to_eye @ projection).reshape(16).copy()
    o = H.GraphicsOptions()
    o.view_distance = VIEW_DISTANCE
    zw = tuple(H.Camera(o, H.Viewport.with_scale(1.0, W, HT)).depth_transform_zw())
    return inv, vp, zw


def options(antialiasing: int):
    """Smoothstep lighting (3) and ambient occlusion with it, the given antialiasing"""
    return oracle.make_options(lighting=3, antialiasing=antialiasing, view_distance=VIEW_DISTANCE)


@functools.lru_cache(maxsize=None)
def oracle_split(name: str, which: str, antialiasing: int):
    """(colour [HT, W, 4] uint16 f16 bit patterns, depth [HT, W] float32) of space `which` = "A" | "B" """
    space = oracle.Space(case(name)[0] if which == "A" else edited(name))
    inv, _, zw = camera(name)
    opt = options(antialiasing)
    points = SAMPLE_POINTS if antialiasing == 2 else [(0.5, 0.5)]
    color = np.zeros((HT, W, 4), np.float32)
    depth = np.zeros((HT, W), np.float64)
    for y in range(HT):
        y0, y1 = -(y / HT * 2.0 - 1.0), -((y + 1) / HT * 2.0 - 1.0)
        for x in range(W):
            x0, x1 = x / W * 2.0 - 1.0, (x + 1) / W * 2.0 - 1.0
            total, d = np.zeros(4, np.float32), np.inf
            for ux, uy in points:
                px, py = (x0 + (x1 - x0) * ux, y0 + (y1 - y0) * uy) if len(points) == 4 else ((x0 + x1) / 2.0, (y0 + y1) / 2.0)
                _, cb, ds = oracle.trace_ray(space, opt, *oracle.project_ndc_into_world(inv, px, py), include_sky=True)
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
def stale_set(name: str, antialiasing: int, flags: int):
    """(S [HT * W] bool, the rectangles) of case `name` from tests/stale_ref.py with expand = 1, under frame A for the depth test"""
    _, vp, _ = camera(name)
    r = stale_ref.rects(vp, W, HT, boxes(name), 1)
    if flags & stale_ref.DEPTH_TEST:
        bits, depth = oracle_split(name, "A", antialiasing)
        s = stale_ref.stale_mask(W, HT, r, bits, depth, flags)
    else:
        s = stale_ref.stale_mask(W, HT, r)
    s.setflags(write=False)
    return s, r
