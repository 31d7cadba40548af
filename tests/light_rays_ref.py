"""The restatement behind the light-ray tests: Space::compute_light::<LightUpdateCubeInfo> (all-is-cubes/src/space/light/updater.rs:
368-530, 770-895; light/debug.rs) as the plain recursion it is in the reference, over what the oracle exports -- the chart, the derived properties of
the blocks, the PackedLight table -- and impl Wireframe for LightUpdateCubeInfo in f64.

The walk here keeps what decides the records: which bundles are visited, alpha along each root path, the direction weights, and `cost`, which counts
every bundle visited within the distance and every branch of `traverse` taken. It does not add up the light; the texel and the cost are the oracle's to
give (oracle.compute_light), and `cost` is what pins this file to it: a walk that visits another bundle or takes another branch has another cost.

Arithmetic: alpha is f32. It is held as a Python float that is always an f32 value; a product or difference of two f32 values formed in f64 and
rounded to f32 once is the f32 operation (53 >= 2 * 24 + 2 bits). (weight * direction_weights).sum() is only ever compared with 0: the chart's weights
are not negative, so it is positive iff a selected weight is. light_from_struck_face is np.float32 arithmetic in the reference's order."""
import math
import sys

import numpy as np

import oracle
from all_is_cubes_amd import abi

NORMALS = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1))  # nx ny nz px py pz
BOX_COLOR = (np.float32(0.8), np.float32(0.8), np.float32(1.0))

_chart = None


def chart():
    """(weight masks, children) of the chart as Python lists: bit f of a mask = the bundle's weight towards face f is positive."""
    global _chart
    if _chart is None:
        w, c = oracle.light_chart()
        assert (w >= 0).all()
        masks = ((w > 0) << np.arange(6)).sum(axis=1).astype(np.int64).tolist()
        _chart = (masks, c.astype(np.int64).tolist())
    return _chart


def _f32(x: float) -> float:
    return float(np.float32(x))


class Tables:
    """What the walk reads of a flat space: taken once per space."""

    def __init__(self, sp):
        d = oracle.compute_derived(oracle.Space(sp))
        self.lo = tuple(int(v) for v in sp.lo)
        self.size = tuple(int(v) for v in sp.size)
        self.grid = np.asarray(sp.block_index).astype(np.int64).tolist()
        self.light = np.ascontiguousarray(sp.light, np.uint8).reshape(*self.size, 4)
        self.visible = d["visible"].tolist()
        self.opaque = d["opaque"].tolist()
        self.all_opaque = d["opaque"].all(axis=1).tolist()
        self.emits = (d["emission"] != 0).any(axis=1).tolist()
        self.emission = d["emission"].astype(np.float32)
        colors = np.concatenate([d["face_colors"], d["color"][:, None, :]], axis=1).astype(np.float32)  # [block][face 0..5, 6 = Within]
        self.colors = colors.copy()
        self.colors[:, :, :3] = np.minimum(colors[:, :, :3], np.float32(1.0))  # Rgba::clamp (color.rs:692-697)
        self.alpha = self.colors[:, :, 3].astype(np.float64).tolist()
        self.lut = oracle.packed_light_lut()

    def rel(self, cube):
        r = (cube[0] - self.lo[0], cube[1] - self.lo[1], cube[2] - self.lo[2])
        return r if 0 <= r[0] < self.size[0] and 0 <= r[1] < self.size[1] and 0 <= r[2] < self.size[2] else None


def compute(t: Tables, cube, maximum_distance: int):
    """(records, cost, outside) of one cube: records are (trigger_cube, value_cube, value [4] u8, light_from_struck_face [3] f32) in the order the
    reference pushes them."""
    masks, children = chart()
    cube = tuple(int(v) for v in cube)
    r0 = t.rel(cube)
    if r0 is None:
        return [], 0, True
    b0 = t.grid[r0[0]][r0[1]][r0[2]]
    if t.all_opaque[b0]:
        return [], 0, False  # updater.rs:385-389: no walk
    # directions_to_seek_light (updater.rs:668-690)
    if t.visible[b0]:
        m0 = 63
    else:
        vis, emi = [False] * 6, [False] * 6
        for f in range(6):
            r = t.rel((cube[0] + NORMALS[f][0], cube[1] + NORMALS[f][1], cube[2] + NORMALS[f][2]))
            if r is not None:
                b = t.grid[r[0]][r[1]][r[2]]
                vis[f], emi[f] = t.visible[b], t.emits[b]
        m0 = sum(1 << f for f in range(6) if vis[(f + 3) % 6] or emi[f])
    max2 = maximum_distance * maximum_distance
    records = []
    cost = 0

    def walk(node, c, fe, alpha, m):
        nonlocal cost
        if not (masks[node] & m):
            return
        dx, dy, dz = c[0] - cube[0], c[1] - cube[1], c[2] - cube[2]
        if dx * dx + dy * dy + dz * dz > max2:
            return
        cost += 1
        r = t.rel(c)
        if r is None:
            return
        b = t.grid[r[0]][r[1]][r[2]]
        if t.visible[b]:  # LightBuffer::traverse
            hit_opaque_face = t.opaque[b][fe] if fe >= 0 else t.all_opaque[b]
            if hit_opaque_face and fe < 0:
                return  # direction_weights = 0, alpha = 0
            hit_alpha = t.alpha[b][fe if fe >= 0 else 6]
            if hit_alpha > 0.0 and fe >= 0:
                n = NORMALS[fe]
                light_cube = (c[0] + n[0], c[1] + n[1], c[2] + n[2])
                cost += 10
                if hit_opaque_face:
                    lr = t.rel(light_cube)
                    assert lr is not None  # the cube the bundle came from
                    stored = t.light[lr]
                    sc = t.colors[b, fe]
                    sv = t.lut[stored[:3]]
                    refl = (sc[:3] * sv).astype(np.float32)
                    refl = np.where(np.isnan(refl), np.float32(0), refl)  # PositiveSign's product
                    refl = (refl * sc[3]).astype(np.float32)
                    refl = np.where(np.isnan(refl), np.float32(0), refl)
                    records.append((c, light_cube, stored.copy(), (t.emission[b] + refl).astype(np.float32)))
                    alpha = 0.0
                else:
                    alpha = _f32(alpha * _f32(1.0 - hit_alpha))
            if hit_alpha < 1.0:
                cost += 10
                alpha = _f32(alpha * _f32(1.0 - hit_alpha))
        if not alpha > 0.0:
            return
        ch = children[node]
        for f in range(6):
            if ch[f]:
                n = NORMALS[f]
                walk(ch[f], (c[0] + n[0], c[1] + n[1], c[2] + n[2]), (f + 3) % 6, alpha, m)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4000))
    try:
        walk(0, cube, -1, 1.0, m0)
    finally:
        sys.setrecursionlimit(limit)
    return records, cost, False


def records_array(records) -> np.ndarray:
    out = np.zeros(len(records), abi.LIGHT_RAY_DTYPE)
    for i, (trigger, value_cube, value, colour) in enumerate(records):
        out[i] = (trigger, value_cube, value, colour)
    return out


def batch(t: Tables, cubes, maximum_distance: int, capacity=None):
    """What aic_light_rays answers for the batch, except `result` (left 0: the oracle's to give): (infos, rays stored, lines stored, totals)."""
    infos = np.zeros(len(cubes), abi.LIGHT_CUBE_INFO_DTYPE)
    per_cube = []
    first = 0
    for k, cube in enumerate(cubes):
        recs, cost, outside = compute(t, cube, maximum_distance)
        arr = records_array(recs)
        stored = capacity is None or first + len(arr) <= capacity
        infos[k] = (tuple(int(v) for v in cube), (0, 0, 0, 0), cost, len(arr), first, (abi.LIGHT_CUBE_STORED if stored else 0) | (abi.LIGHT_CUBE_OUTSIDE if outside else 0))
        per_cube.append(arr if stored else None)
        first += len(arr)
    kept = [a for a in per_cube if a is not None]
    rays = np.concatenate(kept) if kept else np.zeros(0, abi.LIGHT_RAY_DTYPE)
    lines = [wireframe(infos[k]["cube"], a) for k, a in enumerate(per_cube) if a is not None]
    lines = np.concatenate(lines) if lines else np.zeros(0, abi.LINE_VERTEX_DTYPE)
    return infos, rays, lines, (first, 12 * len(cubes) + 29 * first)


# ---- impl Wireframe for LightUpdateCubeInfo (light/debug.rs:50-95), f64 ----

# Aab::wireframe_points (aab.rs:569-588): pairs of octants, a set bit = the upper bound on that axis (bit 2 x, 1 y, 0 z)
BOX_EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))


def _box(cube, d, colour, out):
    for edge in BOX_EDGES:
        for corner in edge:
            out.append(([(float(cube[a]) + 1.0) + d if (corner >> (2 - a)) & 1 else float(cube[a]) - d for a in range(3)], colour))


def _length(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _cross(a, o):
    return [a[1] * o[2] - a[2] * o[1], a[2] * o[0] - a[0] * o[2], a[0] * o[1] - a[1] * o[0]]


def _arrow(lit, trigger, value_cube, colour, out):
    """Ray::wireframe_points (all-is-cubes-base/src/raycast/ray.rs:115-158) of Ray::new(lit.center(), hit_point - lit.center())"""
    origin = [float(lit[a]) + 0.5 for a in range(3)]
    hit = [(float(trigger[a]) + 0.5) * 0.5 + (float(value_cube[a]) + 0.5) * 0.5 for a in range(3)]
    direction = [hit[a] - origin[a] for a in range(3)]
    tip = [origin[a] + direction[a] for a in range(3)]
    out.append((origin, colour))
    out.append((tip, colour))
    length = _length(direction)
    if not length > 0.0:
        return
    norm = [direction[a] / length for a in range(3)]
    head_length = min(length * 0.25, 0.125)
    head_width = head_length * 0.25
    base = [tip[a] - norm[a] * head_length for a in range(3)]
    perp1 = _cross(norm, [0.0, 1.0, 0.0])
    if abs(_length(perp1) - 1.0) > 1e-2:
        perp1 = _cross(norm, [1.0, 0.0, 0.0])
    perp2 = _cross(norm, perp1)

    def circle(step):
        ang = float(step) * (math.tau / 8.0)
        s, c = math.sin(ang), math.cos(ang)
        return [(base[a] + (perp1[a] * head_width) * s) + (perp2[a] * head_width) * c for a in range(3)]

    for step in range(8):
        p, q = circle(step), circle(step + 1)
        out.extend([(p, colour), (tip, colour), (p, colour), (q, colour)])


def wireframe(cube, rays) -> np.ndarray:
    """[2 * (12 + 29 n)] LINE_VERTEX_DTYPE: positions cast to f32 last, colours (0.8, 0.8, 1, 1) and light_from_struck_face with alpha 1"""
    verts = []
    _box(cube, 0.1, BOX_COLOR, verts)
    for r in rays:
        _box(r["value_cube"], 0.01, BOX_COLOR, verts)
        _arrow(cube, r["trigger_cube"], r["value_cube"], tuple(r["light_from_struck_face"]), verts)
    out = np.zeros(len(verts), abi.LINE_VERTEX_DTYPE)
    out["position"] = np.array([p for p, _ in verts], np.float64).astype(np.float32)
    out["color"][:, :3] = np.array([c for _, c in verts], np.float32)
    out["color"][:, 3] = 1.0
    return out


# ---- the scenes and cubes the tests share (tests/test_light_rays_cpu.py, tests/test_gpu_light_rays.py) ----

LAMP_EMISSION = (10.0, 5.0, 0.0)
LAMP_COLOR = (1.0, 0.05, 0.05, 1.0)


def closed_cell_space():
    """3 x 3 x 3: the centre is air, the 26 cubes around it are opaque atoms, the face neighbour towards -X emits. A walk from the centre ends at its six
    face neighbours: exactly six records, each known by hand."""
    from all_is_cubes_amd import flat
    sp = flat.FlatSpace((0, 0, 0), (3, 3, 3))
    sp.set_sky_uniform((1.0, 1.0, 1.0))
    sp.add_block(flat.air())
    wall = sp.add_block(flat.atom((0.5, 0.25, 0.75, 1.0)))
    lamp = sp.add_block(flat.atom(LAMP_COLOR, LAMP_EMISSION))
    sp.block_index[...] = wall
    sp.set((1, 1, 1), 0)
    sp.set((0, 1, 1), lamp)
    sp.light[...] = (0, 0, 0, flat.STATUS_UNINITIALIZED)
    return sp


_scenes = {}


def scene(name: str):
    """(lit flat space, Tables) of "closed_cell", "light_spread" or "light_on_slab": lit once by the oracle's fast_evaluate_light + evaluate_light(1)"""
    if name not in _scenes:
        from tests import scenes
        sp = {"closed_cell": closed_cell_space, "light_spread": scenes.light_spread_space, "light_on_slab": scenes.light_on_slab_space}[name]()
        oracle.evaluate_light(sp, maximum_distance=30, fast=True, epsilon=1, batch=32, hb_width=16)
        _scenes[name] = (sp, Tables(sp))
    return _scenes[name]


def all_cubes(sp):
    lo, size = sp.lo, sp.size
    return [(lo[0] + x, lo[1] + y, lo[2] + z) for x in range(size[0]) for y in range(size[1]) for z in range(size[2])]


# case name -> (scene, cubes, maximum_distance)
def cases():
    spread, slab = scene("light_spread")[0], scene("light_on_slab")[0]
    return {
        "closed_cell": ("closed_cell", [(1, 1, 1)], 6),
        "spread_6": ("light_spread", all_cubes(spread)[::2], 6),
        # the cube above each source, beside a pillar, over the floor's corner, in the open top layer, on the faces of the space
        "spread_30": ("light_spread", [(-2, 3, 0), (-3, 0, 1), (1, 0, 0), (-10, -10, 0), (0, 0, 3), (9, 9, 3), (-3, -1, 2), (4, -5, 1)], 30),
        "slab_6": ("light_on_slab", all_cubes(slab)[::3], 6),
        # around the slabs: recursive blocks, and faces that are neither clear nor opaque
        "slab_30": ("light_on_slab", [(-3, -3, 1), (-2, -3, 0), (3, 3, 1), (0, 0, 2)], 30),
        # an opaque origin (the floor); an invisible origin with no visible neighbour (every direction weight 0); cubes on the space's faces; cubes outside it
        "edges": ("light_spread", [(0, 0, -1), (5, 5, 2), (-10, 0, 0), (9, -10, 3), (-11, 0, 0), (0, 0, 4), (100, 100, 100), (0, 1, 0)], 6),
    }


_answers = {}


def answer(case: str):
    """(infos with the oracle's result, rays, lines, totals) of a case, everything stored: computed once. The restatement's cost is checked against
    oracle.compute_light for every cube inside the space -- that is what pins the walk above to the oracle."""
    if case not in _answers:
        name, cubes, md = cases()[case]
        sp, t = scene(name)
        infos, rays, lines, totals = batch(t, cubes, md)
        osp = oracle.Space(sp)
        for k, cube in enumerate(cubes):
            if infos[k]["flags"] & abi.LIGHT_CUBE_OUTSIDE:
                continue
            texel, cost = oracle.compute_light(osp, cube, md)
            assert cost == infos[k]["cost"], (case, cube, cost, int(infos[k]["cost"]))
            infos[k]["result"] = texel
        _answers[case] = (infos, rays, lines, totals)
    return _answers[case]
