"""The block redefinitions shared by tests/test_stale_blocks_cpu.py and tests/test_gpu_stale_blocks.py, on tests/stale_scenes.py's spaces: a space A, the
same space B after ONE block's definition changed (the cube grid and the light volume unchanged), the cubes that hold the block, and the oracle's Split
frame of either. "ghost" is plaza with a second invisible block that is not air, placed in cubes the library marks OPEN (nothing visible around them)
and on the rim of the space. Everything is computed once."""
import functools

import numpy as np

import oracle
from all_is_cubes_amd import flat
from tests import scenes, stale_blocks_ref, stale_cubes_ref
from tests import stale_scenes as S

W, HT = S.W, S.HT
ANTIALIASING = S.ANTIALIASING
GHOST = 6  # the ghost's block index: behind air, floor, red, green, slab, wall
# two cubes in mid-air (OPEN), one above them on the top layer and two far corners of the rim (never OPEN); none close to the camera, whose rectangle
# would cover much of the frame and make the test of the stale set's size say little
GHOST_CUBES = [(4, 2, 4), (2, 2, 3), (4, 3, 4), (0, 3, 0), (7, 3, 0)]

# name -> (base scene, block index, its new definition)
REDEFINITIONS = {
    "plaza_recolour": ("plaza", 2, lambda: flat.atom((0.1, 0.2, 0.9, 1.0))),
    "plaza_slab": ("plaza", 2, lambda: scenes.slab_block(1, 2)),
    "plaza_invisible": ("plaza", 3, lambda: flat.atom((0.0, 0.0, 0.0, 0.0))),
    "terrace_recolour": ("terrace", 5, lambda: flat.atom((0.8, 0.7, 0.1, 1.0))),
    "terrace_alpha": ("terrace", 5, lambda: flat.atom((0.3, 0.3, 0.7, 0.5))),
    "terrace_atom": ("terrace", 4, lambda: flat.atom((0.6, 0.2, 0.6, 1.0))),
    "ghost_visible": ("ghost", GHOST, lambda: flat.atom((0.9, 0.6, 0.1, 1.0))),
}
CASES = list(REDEFINITIONS)


@functools.lru_cache(maxsize=None)
def base(scene: str) -> flat.FlatSpace:
    """space A of a base scene, with its light"""
    if scene != "ghost":
        return S.case(scene)[0]
    a = S.case("plaza")[0]
    sp = flat.FlatSpace(a.lo, a.size, blocks=list(a.blocks), sky_kind=a.sky_kind, sky=a.sky.copy(), block_index=a.block_index.copy(), light=a.light.copy())
    assert sp.add_block(flat.atom((0.0, 0.0, 0.0, 0.0), name="ghost")) == GHOST
    for cube in GHOST_CUBES:
        assert sp.block_index[cube] == 0
        sp.set(cube, GHOST)
    scenes._unlit(sp)
    oracle.evaluate_light(sp, maximum_distance=8)
    sp.block_index.setflags(write=False)
    sp.light.setflags(write=False)
    return sp


def scene_of(name: str) -> str:
    return REDEFINITIONS[name][0]


def camera(name: str):
    """S.camera of the redefinition's scene (the ghost scene is seen from plaza's camera)"""
    scene = scene_of(name)
    return S.camera("plaza" if scene == "ghost" else scene)


def eye_target(name: str):
    scene = scene_of(name)
    return S.case("plaza" if scene == "ghost" else scene)[2:]


def block_of(name: str) -> int:
    return REDEFINITIONS[name][1]


@functools.lru_cache(maxsize=None)
def new_block(name: str) -> flat.BlockDef:
    return REDEFINITIONS[name][2]()


@functools.lru_cache(maxsize=None)
def redefined(name: str) -> flat.FlatSpace:
    """B: A's grid and light volume, the one block redefined"""
    scene, index, _ = REDEFINITIONS[name]
    a = base(scene)
    blocks = list(a.blocks)
    blocks[index] = new_block(name)
    return flat.FlatSpace(a.lo, a.size, blocks=blocks, sky_kind=a.sky_kind, sky=a.sky.copy(), block_index=a.block_index, light=a.light)


@functools.lru_cache(maxsize=None)
def boxes(name: str) -> np.ndarray:
    """the runs of the cubes that hold the block, from the restatement"""
    scene, index, _ = REDEFINITIONS[name]
    b, _ = stale_blocks_ref.find(base(scene), [index], 1 << 20)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _split(scene: str, name, antialiasing: int):
    """(colour [HT, W, 4] uint16 f16 bit patterns, depth [HT, W] float32) of A of `scene` (name None) or of B of the redefinition `name`: S.oracle_split's
    composition (raytrace_to_texture.rs:623-675 on oracle.trace_ray's buffers of every sample ray)"""
    if name is None and scene != "ghost":
        return S.oracle_split(scene, "A", antialiasing)
    space = oracle.Space(base(scene) if name is None else redefined(name))
    inv, _, zw = S.camera("plaza" if scene == "ghost" else scene)
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


def oracle_split(name: str, which: str, antialiasing: int):
    """the oracle's Split frame of A or B of the redefinition `name`"""
    return _split(scene_of(name), None if which == "A" else name, antialiasing)


@functools.lru_cache(maxsize=None)
def stale_set(name: str, expand: int):
    """S [HT * W] bool: the pixels inside the rectangle of a cube that holds the block, grown by `expand`"""
    _, vp, _ = camera(name)
    b = boxes(name)
    s = stale_cubes_ref.stale_mask(W, HT, stale_cubes_ref.rects(vp, W, HT, b, (), expand), len(b))
    s.setflags(write=False)
    return s
