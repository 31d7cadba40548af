"""The restatement of the cube grid's tags (tests/cube_tags_ref.py) against the definition written out as loops, its class rule on the awkward
blocks, and -- from the model alone, no device -- that the sequences tests/test_gpu_cube_tags.py runs meet the cases they are there for."""
import copy

import numpy as np
import pytest

from all_is_cubes_amd import flat
from tests import cube_tags_ref as ref
from tests import test_gpu_cube_tags as cases
from tests.test_gpu_first_lookup import shell_block
from tests.test_gpu_open_cubes import boundary_space, open_mask


def brute_force_open(sp):
    """The definition, cube by cube: invisible, not on the outermost layer, six invisible face neighbours."""
    cls = [ref.block_class(b) for b in sp.blocks]
    sx, sy, sz = sp.block_index.shape
    m = np.zeros((sx, sy, sz), bool)
    for x in range(sx):
        for y in range(sy):
            for z in range(sz):
                if cls[sp.block_index[x, y, z]] != 0:
                    continue
                if x in (0, sx - 1) or y in (0, sy - 1) or z in (0, sz - 1):
                    continue
                m[x, y, z] = all(cls[sp.block_index[x + dx, y + dy, z + dz]] == 0
                                 for dx, dy, dz in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)))
    return m


@pytest.mark.parametrize("size", ((1, 1, 1), (2, 5, 5), (3, 3, 3), (1, 9, 9), (3, 3, 40), (9, 7, 11)), ids=lambda s: "x".join(map(str, s)))
def test_the_open_set_is_the_definition(size):
    rng = np.random.default_rng(sum(size))
    n_open = 0
    for fill in (0.0, 0.02, 0.1, 0.4):
        sp, ix = cases.scene(size)
        n = int(np.prod(size))
        sp.block_index.reshape(-1)[...] = np.where(rng.random(n) < fill, rng.choice([ix["visible"], ix["recursive"], ix["glow"], ix["ghost"]], n),
                                                   rng.choice([ix["air"], ix["air"], ix["unseen"], ix["tinted"], ix["hollow"]], n))
        want = brute_force_open(sp)
        grid = ref.tagged_grid(sp)
        assert ((grid >> ref.TAG_SHIFT == ref.TAG_OPEN) == want).all() and (ref.open_cubes(sp) == want).all()
        assert ((grid & ref.INDEX_MASK) == sp.block_index).all()
        assert ((grid >> ref.TAG_SHIFT)[~want] == ref.classes(sp.blocks)[sp.block_index][~want] + 1).all()
        n_open += int(want.sum())
    assert (n_open > 0) == (min(size) >= 3)
    if size == (3, 3, 3):
        assert brute_force_open(cases.small_space(size, False)).sum() == 1


def test_the_open_set_is_open_mask_on_the_boundary_scene():
    sp = boundary_space()
    assert (ref.open_cubes(sp) == open_mask(sp)).all() and open_mask(sp).sum() > 100
    assert ((ref.tagged_grid(sp) >> ref.TAG_SHIFT == ref.TAG_OPEN) == open_mask(sp)).all()


def test_the_class_rule_on_the_awkward_blocks():
    assert ref.block_class(flat.air()) == 0
    assert ref.block_class(flat.atom((0.3, 0.9, 0.4, 0.0))) == 0  # alpha 0 and a colour: invisible
    assert ref.block_class(flat.atom((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.1))) == 1  # alpha 0 and an emission: visible
    assert ref.block_class(flat.atom((0.0, 0.0, 0.0, 0.001))) == 1
    assert ref.block_class(cases.hollow_block()) == 0  # resolution 1, the stored volume does not contain [0, 0, 0]: AIR
    pal = np.stack([flat.evoxel((0, 0, 0, 0)), flat.evoxel((0.5, 0.5, 0.5, 1.0))])
    assert ref.block_class(flat.voxel_block(1, np.ones((1, 1, 1), np.uint16), pal)) == 1  # resolution 1: its one stored voxel, not palette[0]
    assert ref.block_class(flat.voxel_block(1, np.zeros((1, 1, 1), np.uint16), pal)) == 0
    assert ref.block_class(cases.ghost_block()) == 2  # recursive, whatever its voxels show
    assert ref.block_class(shell_block(4)) == 2
    # ... so a cube next to a recursive block of invisible voxels is never open, and one next to the others is
    sp, ix = cases.scene((5, 5, 5))
    for name, opens in (("ghost", False), ("glow", False), ("tinted", True), ("hollow", True), ("unseen", True)):
        sp.block_index[...] = ix["air"]
        sp.block_index[2, 2, 3] = ix[name]
        assert ref.open_cubes(sp)[2, 2, 2] == opens and ref.open_cubes(sp)[2, 2, 3] == opens, name
        assert ref.tagged_grid(sp)[2, 2, 3] == ix[name] | ((0 if opens else ref.classes(sp.blocks)[ix[name]] + 1) << ref.TAG_SHIFT)
    table = sp.blocks + [flat.air()] * 11
    words = ref.cls_words(table)
    assert len(words) == 2 and [(int(words[i // 16]) >> (2 * (i % 16))) & 3 for i in range(len(table))] == [ref.block_class(b) for b in table]
    assert len(ref.cls_words(table[:16])) == 1 and len(ref.cls_words(table[:17])) == 2


def test_diff_names_the_kind_of_difference():
    sp = boundary_space()
    want = ref.tagged_grid(sp)
    got = want.copy()
    assert ref.n_differences(ref.diff(got, want)) == 0
    got[4, 3, 3] |= 1 << ref.TAG_SHIFT  # an open cube left at INVISIBLE
    got[5, 3, 3] &= ref.INDEX_MASK  # the cube next to the visible atom marked OPEN
    got[1, 1, 1] = 2 | (ref.TAG_VISIBLE << ref.TAG_SHIFT)
    d = ref.diff(got, want)
    assert d == {"stale OPEN": (1, [(5, 3, 3)]), "missed OPEN": (1, [(4, 3, 3)]), "other": (1, [(1, 1, 1)])}
    assert ref.diff(got, want, tagged=False)["other"][0] == 3


def walk(sp0, steps):
    """What a sequence does, from the model alone: per step, the facts the cases are about."""
    sp = copy.deepcopy(sp0)
    facts = []
    for s in steps:
        before, open_before, cls_before = sp.block_index.copy(), ref.open_cubes(sp), ref.classes(sp.blocks)
        f = dict(what=s.what, layer_1=False, outside=False, adjacent=False, up=False, down=False)
        if s.op[0] == "cubes":
            local = s.op[1].astype(np.int64) - np.array(sp.lo)
            inside = ((local >= 0) & (local < np.array(sp.size))).all(axis=1)
            f["outside"] = bool((~inside).any())
            named = {}
            for i, r in enumerate(map(tuple, local)):  # no cube twice with two values
                value = (None if s.op[2] is None else int(s.op[2][i]), None if s.op[3] is None else tuple(s.op[3][i]))
                assert named.setdefault(r, value) == value, s.what
        sp = cases.apply_to_model(sp, s.op)
        if s.op[0] == "cubes" and s.op[2] is not None:
            changed = np.argwhere(sp.block_index != before)
            rim = np.minimum(changed, np.array(sp.size) - 1 - changed).min(axis=1) if len(changed) else np.zeros(0, int)
            f["layer_1"] = bool((rim == 1).any())
            f["adjacent"] = bool(len(changed) > 1 and (np.abs(changed[:, None, :] - changed[None, :, :]).sum(axis=2) == 1).any())
        if s.op[0] == "blocks":
            for index, block in s.op[1]:
                if index < len(cls_before) and (before == index).any():  # a block some cube holds
                    f["up"] |= cls_before[index] == 0 and ref.block_class(block) != 0
                    f["down"] |= cls_before[index] != 0 and ref.block_class(block) == 0
        now = ref.open_cubes(sp)
        f.update(grows=bool((now & ~open_before).any()), shrinks=bool((open_before & ~now).any()), n_open=int(now.sum()),
                 fill=cases.visible_fill(sp))
        facts.append(f)
    return sp, facts


def some(facts, key):
    return any(f[key] for f in facts)


def test_the_scripted_sequences_are_not_vacuous():
    sp0, steps = cases.scripted_updates()
    _, facts = walk(sp0, steps)
    for key in ("grows", "shrinks", "layer_1", "outside", "adjacent"):
        assert some(facts, key), key
    assert facts[0]["shrinks"] and not facts[0]["grows"] and facts[1]["grows"] and not facts[1]["shrinks"]  # the block into the open region, and out
    assert facts[0]["n_open"] == facts[1]["n_open"] - 7
    assert facts[2]["grows"] and not facts[2]["shrinks"] and facts[2]["n_open"] == facts[1]["n_open"] + 7  # one the upload itself had closed
    assert [len(s.op[1]) for s in steps[-len(cases.BATCH_LENGTHS):]] == list(cases.BATCH_LENGTHS)
    for s in steps[-len(cases.BATCH_LENGTHS):]:
        assert len(np.unique(s.op[1], axis=0)) == len(s.op[1])
    line = next(s for s in steps if "line of 11" in s.what)
    assert len(line.op[1]) == 11 and {int(z) - cases.LO[2] for z in line.op[1][:, 2]} == set(range(11))
    outside = next(f for f in facts if "outside the space" in f["what"])
    assert outside["outside"] and outside["shrinks"]  # the cubes beside them on the outermost layer closed their neighbours on layer 1
    assert all(f["n_open"] > 0 for f in facts)
    # every step marked as leaving the grid alone does so in the model too
    sp = copy.deepcopy(sp0)
    for s in steps:
        g = ref.tagged_grid(sp)
        sp = cases.apply_to_model(sp, s.op)
        assert not s.unchanged or (ref.tagged_grid(sp) == g).all(), s.what

    sp0, steps = cases.scripted_replacements()
    _, facts = walk(sp0, steps)
    for key in ("grows", "shrinks", "up", "down"):
        assert some(facts, key), key
    assert facts[1]["n_open"] == 0 and facts[1]["up"] and facts[2]["down"] and facts[2]["n_open"] > 100  # the block most cubes hold, there and back
    sp = copy.deepcopy(sp0)
    for s in steps:
        g = ref.tagged_grid(sp)
        sp = cases.apply_to_model(sp, s.op)
        assert not s.unchanged or (ref.tagged_grid(sp) == g).all(), s.what


@pytest.mark.parametrize("seed", cases.seeds(4))
def test_the_random_sequences_are_not_vacuous(seed):
    sp0, steps = cases.random_sequence(seed)
    assert len(steps) == cases.N_RANDOM_STEPS and 0.03 <= cases.visible_fill(sp0) <= 0.10
    _, facts = walk(sp0, steps)
    print(seed, {k: sum(bool(f[k]) for f in facts) for k in ("grows", "shrinks", "layer_1", "outside", "adjacent", "up", "down")},
          "open", min(f["n_open"] for f in facts), max(f["n_open"] for f in facts), "fill", min(f["fill"] for f in facts), max(f["fill"] for f in facts))
    for key in ("grows", "shrinks", "layer_1", "outside", "adjacent", "up", "down"):
        assert some(facts, key), key
    for f in facts:
        # neither direction of error could hide: something is open, something is visible, and the scene stays sparse
        assert f["n_open"] >= 1 and 0.03 <= f["fill"] <= 0.10, f
    for s in steps:
        if s.op[0] == "cubes":
            assert 1 <= len(s.op[1]) <= 60 and len(np.unique(s.op[1], axis=0)) == len(s.op[1]), s.what
    marked = [k + 1 for k, s in enumerate(steps) if s.fresh]
    assert marked == [10, 20, 30, 40] and all((s.view is not None) == s.fresh for s in steps)
    # the same seed gives the same sequence
    again = cases.random_sequence(seed)[1]
    assert all(a.what == b.what and a.op[0] == b.op[0] for a, b in zip(steps, again))
