"""cursor_raycast (all-is-cubes/src/character/cursor.rs:26-107) restated in plain Python over the CPU oracle's Raycaster -- what aic_cursor_raycast must
reproduce field for field, f64 by bit pattern. The outer walk is oracle.raycast(.., include_exit=False); a block's voxels are walked by the sub-ray of
RaycastStep::recursive_raycast: its origin is computed here in NumPy f64, one rounding per operation, and checked against oracle.recursive_raycast
wherever the unbounded Raycaster that function steps reaches the cube. The normalisation and PositiveSign::new_clamped are NumPy f64 too. What
"selectable" means is the rule of include/aic_hip.h (AIC_BLOCK_UNSELECTABLE, AIC_BLOCK_VOXEL_SELECTABLE), read from the flat space's BlockDefs.

Also the case list -- scenes of at most 8^3 cubes with blocks of resolution 2 to 16, and ray batches -- that the CPU test checks for coverage and the
GPU test runs on the device, and the reference's own seven tests (cursor.rs:310-436) as scenes made here."""
import numpy as np

import oracle
from all_is_cubes_amd import abi, flat
from tests.exposure_ref import FACE_NORMALS, ODD_RAYS, light_outside

f64 = np.float64
WITHIN, NX, NY, NZ, PX, PY, PZ = range(7)  # Face7 discriminants

# what happened to a ray, for the coverage check
NONE_NEVER, NONE_LEFT, NONE_DISTANCE = "none: never meets the bounds", "none: leaves the bounds", "none: over maximum_distance"
PASSED_UNSELECTABLE, PASSED_MISSED, PASSED_EMPTY = "passed: unselectable block", "passed: sub-ray missed the voxel bounds", "passed: no selectable voxel"
SKIPPED_AIR_VOXEL, HIT_INVISIBLE_FLAGGED, SKIPPED_VISIBLE_FLAGGED = "skipped: invisible voxel, default rule", "hit: invisible voxel flagged selectable", "skipped: visible voxel flagged unselectable"
HIT_SINGLE, HIT_VOXEL, HIT_OTHER_FACE = "hit: single voxel", "hit: voxel", "hit: face_selected != face_entered"
HIT_WITHIN, SELECTED_WITHIN, PRECEDING_OUTSIDE, HIT_AT_MAXIMUM = "hit: Within, no preceding", "hit: face_selected Within in a voxel block", "hit: preceding cube outside the bounds", "hit: t_distance == maximum_distance"
REQUIRED = [NONE_NEVER, NONE_LEFT, NONE_DISTANCE, PASSED_UNSELECTABLE, PASSED_MISSED, PASSED_EMPTY, SKIPPED_AIR_VOXEL, HIT_INVISIBLE_FLAGGED,
            SKIPPED_VISIBLE_FLAGGED, HIT_SINGLE, HIT_OTHER_FACE, HIT_WITHIN, SELECTED_WITHIN, PRECEDING_OUTSIDE, HIT_AT_MAXIMUM]


def normalize(d) -> np.ndarray:
    """Vector3D::normalize: self / self.length()"""
    d = np.asarray(d, f64)
    with np.errstate(all="ignore"):
        length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        return d / length


def invisible(e) -> bool:
    return bool(e[3] == 0 and e[4] == 0 and e[5] == 0 and e[6] == 0)


def voxel_selectable(b: flat.BlockDef, entry: int) -> bool:
    """Evoxel::selectable of a palette entry: as given, or by the default rule (selectable iff not invisible)"""
    if b.voxel_selectable is not None:
        return bool(b.voxel_selectable[entry])
    return not invisible(b.palette[entry])


def single_voxel(b: flat.BlockDef):
    """Evoxels::single_voxel (voxel_storage.rs:364-385): the palette entry, -1 for the AIR outside the stored volume, or None for a block with voxels"""
    if b.is_one:
        return 0
    if b.resolution != 1:
        return None
    inside = b.voxels.size > 0 and all(b.vlo[a] <= 0 < b.vlo[a] + b.voxels.shape[a] for a in range(3))
    return int(b.voxels[tuple(-int(v) for v in b.vlo)]) if inside else -1


class Scene:
    """What the raycast reads of a flat space."""

    def __init__(self, sp: flat.FlatSpace):
        self.sp = sp
        self.block_sky = oracle.block_sky(oracle.Space(sp))
        self.lo = tuple(int(v) for v in sp.lo)
        self.hi = tuple(int(v) for v in sp.hi)
        self.max_steps = sum(int(v) for v in sp.size) + 3

    def inside(self, c) -> bool:
        return all(self.lo[a] <= int(c[a]) < self.hi[a] for a in range(3))

    def light(self, cube) -> np.ndarray:
        """Space::get_light"""
        if self.inside(cube):
            return np.asarray(self.sp.light[tuple(int(cube[a]) - self.lo[a] for a in range(3))], np.uint8)
        return light_outside(self.block_sky, self.lo, self.hi, [int(v) for v in cube])

    def sub_steps(self, o, d, cube, b: flat.BlockDef):
        """step.recursive_raycast(ray, resolution, voxels.bounds()).0"""
        res = f64(b.resolution)
        sub_o = np.array([(f64(o[a]) - f64(int(cube[a]))) * res for a in range(3)], f64)
        vlo = tuple(int(v) for v in b.vlo)
        vhi = tuple(vlo[a] + int(b.voxels.shape[a]) for a in range(3))
        limit = sum(b.voxels.shape) + 3
        steps, _ = oracle.raycast(sub_o, d, (vlo, vhi), include_exit=True, max_steps=limit)
        # the oracle's own recursive_raycast, which steps an unbounded Raycaster to the cube: the same sub-ray wherever that reaches it
        free, _ = oracle.raycast(o, d, None, max_steps=48)
        at = [i for i, st in enumerate(free) if tuple(int(v) for v in st["cube"]) == tuple(int(v) for v in cube)]
        if at:
            theirs, _, their_o = oracle.recursive_raycast(o, d, at[0], int(b.resolution), (vlo, vhi), max_steps=limit)
            assert their_o.tobytes() == sub_o.tobytes() and theirs.tobytes() == steps.tobytes()
        return steps, vlo, vhi

    def raycast(self, ray, maximum_distance: float, outcomes=None) -> np.ndarray:
        """cursor_raycast -> one CURSOR_HIT_DTYPE record, all zero for None"""
        sp = self.sp
        rec = np.zeros((), abi.CURSOR_HIT_DTYPE)
        note = outcomes.add if outcomes is not None else (lambda _: None)
        o = np.asarray(ray[:3], f64)
        d = normalize(ray[3:])
        steps, _ = oracle.raycast(o, d, (self.lo, self.hi), include_exit=False, max_steps=self.max_steps)
        for n, st in enumerate(steps):
            t = f64(st["t_distance"])
            if t > maximum_distance:
                note(NONE_DISTANCE)
                return rec
            cube = [int(v) for v in st["cube"]]
            if not self.inside(cube):
                continue
            index = int(sp.block_index[tuple(cube[a] - self.lo[a] for a in range(3))])
            b = sp.blocks[index]
            if b.is_air or not b.selectable:
                if not b.is_air:
                    note(PASSED_UNSELECTABLE)
                continue
            face = int(st["face"])
            face_selected, voxel, vlo, vsize, res = face, (0, 0, 0), (0, 0, 0), (1, 1, 1), 1
            single = single_voxel(b)
            if single is not None:
                if single < 0 or not voxel_selectable(b, single):
                    if single >= 0 and b.voxel_selectable is not None and not invisible(b.palette[single]):
                        note(SKIPPED_VISIBLE_FLAGGED)
                    continue
                note(HIT_SINGLE)
                if b.voxel_selectable is not None and invisible(b.palette[single]):
                    note(HIT_INVISIBLE_FLAGGED)
            else:
                vsteps, vlo, vhi = self.sub_steps(o, d, cube, b)
                vsize, res = tuple(vhi[a] - vlo[a] for a in range(3)), int(b.resolution)
                if len(vsteps) == 0:
                    note(PASSED_MISSED)
                    continue
                face_selected = int(vsteps[0]["face"])
                found = None
                for vs in vsteps:
                    vc = [int(v) for v in vs["cube"]]
                    if not all(vlo[a] <= vc[a] < vhi[a] for a in range(3)):
                        continue  # get_opt_evoxel: None (the exit step)
                    entry = int(b.voxels[tuple(vc[a] - vlo[a] for a in range(3))])
                    if voxel_selectable(b, entry):
                        found = (vc, entry)
                        break
                    note(SKIPPED_VISIBLE_FLAGGED if b.voxel_selectable is not None and not invisible(b.palette[entry]) else
                         SKIPPED_AIR_VOXEL if b.voxel_selectable is None else "skipped: invisible voxel flagged unselectable")
                if found is None:
                    note(PASSED_EMPTY)
                    continue
                voxel = tuple(found[0])
                note(HIT_VOXEL)
                if b.voxel_selectable is not None and invisible(b.palette[found[1]]):
                    note(HIT_INVISIBLE_FLAGGED)
                if face_selected == WITHIN:
                    note(SELECTED_WITHIN)
            if face_selected != face:
                note(HIT_OTHER_FACE)
            if t == maximum_distance:
                note(HIT_AT_MAXIMUM)
            rec["cube"], rec["face_entered"], rec["face_selected"] = cube, face, face_selected
            rec["point_entered"] = st["intersection_point"]
            rec["distance_to_point"] = t if t > 0 else f64(0.0)  # PositiveSign::new_clamped
            rec["voxel_lo"], rec["voxel_size"], rec["resolution"] = vlo, vsize, res
            rec["hit"], rec["block_index"], rec["voxel"], rec["steps"] = 1, index, voxel, n + 1
            rec["light_hit"] = self.light(cube)
            if face != WITHIN:
                behind = [cube[a] + int(FACE_NORMALS[face][a]) for a in range(3)]
                rec["has_preceding"], rec["preceding_cube"] = 1, behind
                rec["light_preceding"] = self.light(behind)
                if self.inside(behind):
                    rec["preceding_block_index"] = int(sp.block_index[tuple(behind[a] - self.lo[a] for a in range(3))])
                else:
                    rec["preceding_block_index"] = abi.CURSOR_NO_BLOCK
                    note(PRECEDING_OUTSIDE)
            else:
                note(HIT_WITHIN)
            return rec
        note(NONE_NEVER if len(steps) == 0 else NONE_LEFT)
        return rec

    def raycast_all(self, rays, maximum_distance: float, outcomes=None) -> np.ndarray:
        rays = np.asarray(rays, f64).reshape(-1, 6)
        out = np.zeros(len(rays), abi.CURSOR_HIT_DTYPE)
        for i, r in enumerate(rays):
            out[i] = self.raycast(r, maximum_distance, outcomes)
        return out


def field_bytes(records: np.ndarray) -> np.ndarray:
    """[n, bytes]: the bytes of every field of every record, in the struct's order (the four bytes of padding before point_entered are no field)"""
    records = np.atleast_1d(records)
    return np.concatenate([np.ascontiguousarray(records[name]).view(np.uint8).reshape(len(records), records.dtype[name].itemsize) for name in records.dtype.names], axis=1)


def same_records(got: np.ndarray, want: np.ndarray):
    """Every field of every record: integers exactly, f64 by bit pattern -- which is the fields' bytes. Returns the indices that differ."""
    return np.flatnonzero((field_bytes(got) != field_bytes(want)).any(axis=1))


# ---- the reference's seven tests (cursor.rs:286-436) -------------------------------------------------------------------

X_RAY = np.array([-0.5, 0.500001, 0.500001, 1.0, 0.0, 0.0])
SLOPING_RAY = np.array([-0.25, 1.0, 0.5, 1.0, -1.0, 0.0])


def some_block() -> flat.BlockDef:
    return flat.atom((0.5, 0.5, 0.5, 1.0))


def white_unselectable() -> flat.BlockDef:
    b = flat.atom((1.0, 1.0, 1.0, 1.0), name="w")
    b.selectable = False
    return b


def slab(numerator: int, resolution: int) -> flat.BlockDef:
    """make_slab: a two-colour checkerboard filling the lower numerator / resolution of the block; its voxel bounds are [0,0,0] + (r, numerator, r)"""
    pal = np.stack([flat.evoxel((0.2, 0.2, 0.2, 1.0)), flat.evoxel((0.8, 0.8, 0.8, 1.0))])
    vox = (np.indices((resolution, numerator, resolution)).sum(0) % 2).astype(np.uint16)
    return flat.voxel_block(resolution, vox, pal, name="s")


def row_space(*blocks) -> flat.FlatSpace:
    """test_space: an N x 1 x 1 space at the origin holding the given blocks in order"""
    sp = flat.FlatSpace((0, 0, 0), (len(blocks), 1, 1))
    sp.set_sky_octants(np.arange(24, dtype=np.float32).reshape(8, 3) / 8)
    for x, b in enumerate(blocks):
        sp.block_index[x, 0, 0] = sp.add_block(b)
        sp.light[x, 0, 0] = (40 + x, 90 + x, 140 + x, flat.STATUS_VISIBLE)
    return sp


def reference_tests():
    """[(name, make_space, ray, maximum_distance, expected)]: expected is None, or a dict of the fields the reference asserts"""
    inf = float("inf")
    return [
        ("simple_hit_after_air", lambda: row_space(flat.air(), some_block()), X_RAY, inf, dict(cube=(1, 0, 0), face_selected=NX, block_index=1)),
        ("maximum_distance_too_short", lambda: row_space(flat.air(), some_block()), X_RAY, 1.0, None),
        ("ignores_not_selectable_atom", lambda: row_space(white_unselectable(), some_block()), X_RAY, inf, dict(cube=(1, 0, 0), block_index=1)),
        ("ignores_not_selectable_voxels", lambda: row_space(slab(1, 2), some_block()), X_RAY, inf, dict(cube=(1, 0, 0), block_index=1)),
        ("hits_selectable_voxels", lambda: row_space(flat.air(), slab(3, 4), some_block()), X_RAY, inf, dict(cube=(1, 0, 0), block_index=1)),
        ("slope_hits_face_of_full_block", lambda: row_space(some_block()), SLOPING_RAY, inf, dict(face_entered=NX, face_selected=NX)),
        ("slope_hits_face_different_from_entered", lambda: row_space(slab(1, 2)), SLOPING_RAY, inf, dict(face_entered=NX, face_selected=PY)),
    ]


# ---- the case list ---------------------------------------------------------------------------------------------------

AIR_I, ATOM, UNSEL_ATOM, GHOST, OFFSET, FLAGGED, SPARSE16, CHECKER, UNSEL_VOXELS, FLAGGED_GLASS, FLAGGED_PAINT = range(11)


def garden_blocks():
    air_v, grey, red = flat.evoxel((0, 0, 0, 0)), flat.evoxel((0.5, 0.5, 0.5, 1.0)), flat.evoxel((0.9, 0.1, 0.1, 0.5))
    glow = flat.evoxel((0, 0, 0, 0), (0.5, 1.0, 2.0))
    rng = np.random.default_rng(11)
    sparse = (rng.random((16, 16, 16)) < 0.04).astype(np.uint16)
    sparse[7:9, 7:9, 7:9] = 2
    unsel_voxels = flat.voxel_block(2, np.ones((2, 2, 2), np.uint16), np.stack([air_v, grey]), name="u")
    unsel_voxels.selectable = False
    glass = flat.atom((0, 0, 0, 0), name="g")  # invisible, selectable
    glass.voxel_selectable = [True]
    paint = flat.atom((0.1, 0.9, 0.1, 1.0), name="p")  # visible, not selectable
    paint.voxel_selectable = [False]
    flagged = flat.voxel_block(2, np.array([[[0, 1], [1, 2]], [[1, 0], [2, 1]]], np.uint16), np.stack([air_v, grey, red]), name="f")
    flagged.voxel_selectable = [True, False, True]  # an invisible voxel that is selectable, a visible one that is not
    return [
        flat.air(),
        flat.atom((0.5, 0.5, 0.5, 1.0)),
        white_unselectable(),
        flat.voxel_block(4, np.indices((4, 4, 4)).sum(0).astype(np.uint16) % 2, np.stack([air_v, flat.evoxel((0.3, 0.2, 0.1, 0.0))]), name="i"),  # all invisible
        flat.voxel_block(8, np.ones((3, 2, 4), np.uint16), np.stack([air_v, grey]), vlo=(2, 3, 1), name="o"),  # a stored volume in a corner of the block
        flagged,
        flat.voxel_block(16, sparse, np.stack([air_v, grey, glow]), name="S"),
        flat.voxel_block(4, np.indices((4, 4, 4)).sum(0).astype(np.uint16) % 2, np.stack([air_v, red]), name="c"),  # AIR and colour, checkered
        unsel_voxels,
        glass,
        paint,
    ]


def garden_space() -> flat.FlatSpace:
    """6 x 5 x 7 cubes at (-2, -1, -3) with every kind of block the rule tells apart, every cube's light texel its own"""
    sp = flat.FlatSpace((-2, -1, -3), (6, 5, 7))
    sp.set_sky_octants(np.array([[0.1 * (o + 1), 0.05 * (8 - o), 0.3 + 0.2 * (o % 3)] for o in range(8)], np.float32))
    for b in garden_blocks():
        sp.add_block(b)
    rng = np.random.default_rng(7)
    kinds = rng.choice(11, size=(6, 5, 7), p=[0.56, 0.04, 0.06, 0.05, 0.06, 0.05, 0.04, 0.05, 0.03, 0.03, 0.03])
    sp.block_index[...] = kinds.astype(np.uint16)
    # a corridor along -Z from the eye of the odd rays, (0.5, 0.5, 3.5): air, then one of each of the blocks a ray is passed over by, then an atom
    for z, k in zip(range(3, -4, -1), (AIR_I, UNSEL_ATOM, GHOST, FLAGGED_PAINT, UNSEL_VOXELS, OFFSET, ATOM)):
        sp.set((0, 0, z), k)
    x, y, z = np.indices((6, 5, 7))
    sp.light[..., 0], sp.light[..., 1], sp.light[..., 2] = 10 + 37 * x, 20 + 41 * y, 30 + 29 * z
    sp.light[..., 3] = np.where(kinds == AIR_I, flat.STATUS_VISIBLE, flat.STATUS_OPAQUE)
    return sp


def random_rays(n: int, seed: int, lo, hi, inside: float = 0.5) -> np.ndarray:
    """origins within the bounds (a share `inside`) or up to 3 cubes around them, aimed at points within the bounds; directions not normalised"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    grow = np.where(rng.random((n, 1)) < inside, 0.0, 3.0)
    origin = rng.uniform(lo - grow, hi + grow)
    target = rng.uniform(lo, hi, (n, 3))
    return np.concatenate([origin, (target - origin) * rng.uniform(0.2, 3.0, (n, 1))], axis=1)


CRAFTED = np.array([
    [0.5, 0.5, 3.5, 0.0, 0.0, -2.0],       # down the corridor: every kind of pass, then the atom
    [0.5, 0.5, 10.0, 0.0, 0.0, -1.0],      # the same from outside
    [9.0, 9.0, 9.0, 1.0, 0.0, 0.0],        # never meets the bounds
    [-5.0, 0.5, 3.5, 1.0, 0.0, 0.0],       # along the open top layer ...
    [0.5, 0.5, -2.5, 0.0, 0.25, 0.0],      # from inside the atom at the corridor's end: Within
    [0.5, 0.5, -2.5, 0.0, 0.0, 0.0],       # ... and with no direction at all
    [0.4, 0.5, -1.6, 0.0, 0.0, -1.0],      # from inside the corner block's stored volume (voxels 2..5, 3..5, 1..5 of 8): face_selected Within
    [0.4, 0.1, -1.6, 0.0, 0.0, -1.0],      # beside that volume: the sub-ray misses it
    [-5.0, 0.5, -2.5, 1.0, 0.0, 0.0],      # onto the space's -X side
], f64)


def garden_rays() -> np.ndarray:
    sp_lo, sp_hi = (-2, -1, -3), (4, 4, 4)
    return np.concatenate([CRAFTED, random_rays(121, 3, sp_lo, sp_hi)])  # 130 rays: two waves and two lanes


def garden_odd_rays() -> np.ndarray:
    return np.concatenate([ODD_RAYS, ODD_RAYS * [1, 1, 1, 1, 1, 1] + [0, 0, -6.0, 0, 0, 0]])


def cases():
    """[(name, scene key, rays [n,6], maximum_distance)]: every scene, batch and distance the tests run. Scenes are made on demand (`scene` caches them)."""
    inf = float("inf")
    out = [(f"garden, {md}", "garden", garden_rays(), md) for md in (inf, 6.0, 2.5)]
    out.append(("garden, odd rays", "garden", garden_odd_rays(), inf))
    out.append(("garden, from far outside", "garden", random_rays(40, 5, (-2, -1, -3), (4, 4, 4), inside=0.0) * [40, 40, 40, 1, 1, 1], inf))
    out.append(("row: the hit at exactly maximum_distance", "row", np.stack([X_RAY, X_RAY * [1, 1, 1, 7, 1, 1]]), 1.5))
    out.append(("row: slabs", "slabs", np.stack([X_RAY, SLOPING_RAY, SLOPING_RAY * [1, 1, 1, 1, -0.25, 1], X_RAY + [0, 0.3, 0, 0, 0, 0]]), inf))
    return out


SPACE_MAKERS = {"garden": garden_space, "row": lambda: row_space(flat.air(), some_block()),
                "slabs": lambda: row_space(slab(1, 2), slab(3, 4), flat.air(), slab(1, 2), some_block())}
_scenes = {}


def scene(key: str) -> Scene:
    if key not in _scenes:
        _scenes[key] = Scene(SPACE_MAKERS[key]())
    return _scenes[key]
