"""GPU tests (-m gpu) of aic_find_block_cubes and aic_pick_stale_blocks: the cubes that hold a re-evaluated block found in the resident cube grid, and
their pixels picked first.

Yardstick: tests/stale_blocks_ref.py, the restatement of DESIGN.md 4.20 in NumPy, composed with tests/stale_cubes_ref.py for the lists. Boxes, every
info field and whole uint32 lists are compared; there is no tolerance anywhere. Grids: tests/test_stale_blocks_cpu.py's, which hold a grid of one entry,
rows as long as a lane's group of 8 entries, 2049 entries (one past a workgroup's 2048) and 10500 entries (six workgroups, runs across their borders).
Scenes, frames and expected sets are made once and shared."""
import ctypes as C

import numpy as np
import pytest

from all_is_cubes_amd import abi, flat
from tests import cube_tags_ref as tags
from tests import stale_block_scenes as B
from tests import stale_blocks_ref as ref
from tests import stale_cubes_ref, stale_ref
from tests import test_gpu_pick as pk
from tests import test_gpu_reproject as rp
from tests import test_gpu_stale as gs
from tests import test_gpu_stale_cubes as gc
from tests import test_stale_blocks_cpu as cpu
from tests.test_gpu_parity import to_abi_options

gpu = pytest.mark.gpu
WORLD, UI = abi.LAYER_WORLD, abi.LAYER_UI
AIC_ERR_INVALID = 1
SENTINEL_WORD = pk.SENTINEL_WORD
INFO_FIELDS = ("n_cubes", "n_runs", "n_written", "merged")


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(0)
    yield c
    c.close()


def found_dict(info):
    assert info.kernel_ms >= 0.0 and info.reserved == 0
    return {**{k: int(getattr(info, k)) for k in INFO_FIELDS}, "bounds": [int(v) for v in info.bounds]}


def check_find(ctx, sp, indices, capacity, what, layer=WORLD):
    want, want_info = ref.find(sp, indices, capacity)
    got, info = ctx.find_block_cubes(layer, indices, capacity)
    assert found_dict(info) == want_info, (what, capacity)
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, capacity, got[:4], want[:4])
    return got, info


def check_capacities(ctx, sp, indices, what, layer=WORLD):
    """every run; capacity exactly n_runs; one less (merged: the one box is the bounds); none"""
    n_runs = ref.find(sp, indices, 1 << 30)[1]["n_runs"]
    for capacity in sorted({n_runs + 9, n_runs, max(n_runs - 1, 0), 0}, reverse=True):
        got, info = check_find(ctx, sp, indices, capacity, what, layer)
        if capacity < n_runs:
            assert info.merged == 1 and len(got) == min(capacity, 1) and (not capacity or got[0].tolist() == list(info.bounds))
    return n_runs


@gpu
@pytest.mark.parametrize("size", cpu.GRIDS)
def test_find_equals_the_restatement_on_the_grids(ctx, size):
    for pattern in cpu.PATTERNS:
        sp, indices = cpu.grid_space(size, pattern)
        ctx.upload_space(WORLD, sp)
        n_runs = check_capacities(ctx, sp, indices, pattern)
        first = ctx.find_block_cubes(WORLD, indices, n_runs + 1)
        again = ctx.find_block_cubes(WORLD, indices, n_runs + 1)
        assert first[0].tobytes() == again[0].tobytes() and found_dict(first[1]) == found_dict(again[1]), "two runs of the same call"
        check_find(ctx, sp, [1, 1, 2, 1], 1 << 16, "duplicates and a second index")
        check_find(ctx, sp, [0, 1, 2], 1 << 16, "all indices")
        check_find(ctx, sp, [], 4, "no index")
    print(size, "ok")


@gpu
def test_find_follows_update_cubes_and_replace_blocks(ctx):
    """the grid after scattered updates (which re-tag cubes and move OPEN marks), and block redefinitions of the same class, visible <-> invisible and
    atom <-> recursive, which leave the grid's indices as they are"""
    from tests import scenes

    sp, _ = cpu.grid_space((5, 7, 300), "random", (0, 0, 0))
    sp = flat.FlatSpace(sp.lo, sp.size, blocks=list(sp.blocks), block_index=sp.block_index.copy())
    ctx.upload_space(WORLD, sp)
    rng = np.random.default_rng(4)
    for step in range(3):
        linear = rng.choice(int(np.prod(sp.size)), 400, replace=False)  # (no cube twice in one call)
        cubes = np.stack(np.unravel_index(linear, sp.size), axis=1).astype(np.int32)
        index = rng.integers(0, 3, 400).astype(np.uint16)
        ctx.update_cubes(WORLD, cubes, index)
        for q, i in zip(cubes, index):
            sp.set(q, int(i))
        for indices in ([1], [2], [0], [1, 2]):
            check_capacities(ctx, sp, indices, f"update {step}")
    for block in (flat.atom((0.2, 0.3, 0.9, 1.0)), flat.atom((0.0, 0.0, 0.0, 0.0)), scenes.slab_block(1, 2), flat.atom((0.5, 0.5, 0.1, 0.5)), flat.atom((0.0, 0.0, 0.0, 0.0)),
                  flat.atom((0.9, 0.1, 0.1, 1.0))):
        ctx.replace_blocks(WORLD, [(1, block)])
        sp.blocks[1] = block
        for indices in ([1], [2], [0]):
            check_capacities(ctx, sp, indices, "replace")
    grid, _, tagged = ctx.probe_cube_grid(WORLD, sp.size, len(sp.blocks))
    assert tagged and ((grid & tags.INDEX_MASK) == sp.block_index).all() and (grid >> tags.TAG_SHIFT).max() >= 1, "the grid carries tags over the model's indices"


@gpu
def test_the_ghost_block_in_open_cubes_is_found(ctx):
    """an invisible block that is not air: its cubes in mid-air are OPEN (tag 0), the others INVISIBLE (tag 1: bit 14 set) -- both match by index"""
    sp = B.base("ghost")
    ctx.upload_space(WORLD, sp)
    grid, _, tagged = ctx.probe_cube_grid(WORLD, sp.size, len(sp.blocks))
    held = sp.block_index == B.GHOST
    assert tagged and set((grid[held] >> tags.TAG_SHIFT).tolist()) == {tags.TAG_OPEN, tags.TAG_INVISIBLE}
    got, info = check_find(ctx, sp, [B.GHOST], 64, "ghost")
    assert info.n_cubes == len(B.GHOST_CUBES)
    for i in range(len(sp.blocks)):
        check_capacities(ctx, sp, [i], f"block {i}")
    check_capacities(ctx, sp, [0, B.GHOST], "air and ghost")


@gpu
def test_a_table_of_16385_blocks_has_plain_entries(ctx):
    """the grid carries no tags then, and indices have bit 14 set: 16384 must not match block 0, nor 16385 % 16384"""
    sp = flat.FlatSpace((-3, 0, 5), (3, 4, 70))
    atom = flat.atom((0.4, 0.4, 0.4, 1.0))
    sp.blocks = [flat.air()] + [atom] * 16384
    rng = np.random.default_rng(9)
    sp.block_index[...] = rng.choice(np.array([0, 1, 16383, 16384], np.uint16), sp.size)
    assert not tags.is_tagged(sp)
    ctx.upload_space(WORLD, sp)
    assert not ctx.probe_cube_grid(WORLD, sp.size, len(sp.blocks))[2]
    for indices in ([16384], [0], [16383, 16384], [1, 0]):
        check_capacities(ctx, sp, indices, str(indices))


@gpu
def test_layer_1(ctx):
    world, _ = cpu.grid_space((2, 5, 51), "random")
    ui, _ = cpu.grid_space((3, 3, 40), "every_other", (1, 2, 3))
    ctx.upload_space(WORLD, world)
    ctx.upload_space(UI, ui)
    try:
        check_capacities(ctx, ui, [1], "ui", UI)
        check_capacities(ctx, world, [1], "world", WORLD)
    finally:
        ctx.clear_space(UI)


# ---- the lists --------------------------------------------------------------------------------------------------------------------------------------

SCENE, BLOCKS = "terrace", [5, 4]  # the wall along the back (8 runs) and the slab


def pick_blocks(ctx, w, h, n, boxes, cubes, blocks, src, order_dev, **kw):
    out = pk.out_words(n)
    info = ctx.pick_stale_blocks(gc.view_projection(w, h), w, h, n, boxes, cubes, WORLD, blocks, src.data_ptr() if src is not None else 0,
                                 order_dev.data_ptr() if order_dev is not None else 0, out.data_ptr(), **kw)
    raw = out.cpu().numpy().view(np.uint32)
    assert (raw[n:] == SENTINEL_WORD).all(), "guard words behind pixels_out[n)"
    assert info.pick.kernel_ms >= 0.0 and info.found.kernel_ms >= 0.0 and info.pick.reserved == 0
    return raw[:n].copy(), gc.info_dict(info.pick), found_dict(info.found)


def check_pick(ctx, sp, w, h, kind, n, boxes, cubes, blocks, src, order_dev, frame, what, max_runs=65536, **kw):
    """the call against the restatement, and against find_block_cubes + pick_stale_cubes on the same context"""
    color, depth = frame
    want, want_pick, want_found = ref.pick_list(sp, blocks, max_runs, gc.view_projection(w, h), w, h, gs.order_of(w, h, kind), n, boxes, cubes, kw.get("expand", 1), color, depth,
                                                kw.get("flags", 0), kw.get("max_stale", 0), kw.get("skip_stale", 0), kw.get("cursor", 0),
                                                picker=lambda m, c: gs.picker_list(w, h, kind, m, c))
    got, got_pick, got_found = pick_blocks(ctx, w, h, n, boxes, cubes, blocks, src, order_dev, max_runs=max_runs, **kw)
    print(f"{w}x{h} {kind} {what}: n {n} max_runs {max_runs} {kw} -> {got_pick} {got_found}; entries differing {int((got != want).sum())}")
    assert got_found == want_found and got_pick == want_pick, what
    assert (got == want).all(), what
    # by composition
    found, _ = ctx.find_block_cubes(WORLD, blocks, max_runs) if n and kw.get("max_stale", 0) else (np.zeros((0, 6), np.int32), None)
    own = np.asarray(boxes if boxes is not None else [], np.int32).reshape(-1, 6)
    out = pk.out_words(n)
    info = ctx.pick_stale_cubes(gc.view_projection(w, h), w, h, n, np.concatenate([own, found]), cubes, src.data_ptr() if src is not None else 0,
                                order_dev.data_ptr() if order_dev is not None else 0, out.data_ptr(), **kw)
    assert gc.info_dict(info) == got_pick and (out.cpu().numpy().view(np.uint32)[:n] == got).all(), (what, "composition")
    return got, got_pick, got_found


@gpu
@pytest.mark.parametrize("kind", gs.ORDERS)
@pytest.mark.parametrize("w,h", [(61, 37), (523, 503)])
def test_lists_equal_the_restatement_and_the_composition(ctx, w, h, kind):
    sp = B.base(SCENE)
    ctx.upload_space(WORLD, sp)
    frame = gc.frame(w, h)
    src_bytes = rp.frame_bytes(*frame)
    src = rp.to_device(src_bytes)
    order_dev = pk.to_device_words(gs.picker_order(w, h)) if kind == "picker" else None
    boxes, cubes = gc.cube_set("257")
    count = w * h
    big = count if count < 5000 else 20000  # picks of a call that wants the whole set: the large frame's set is checked by its size and its first 20000 ranks
    args = (src, order_dev, frame)
    # the found boxes alone, every flag (boxes use the front test only)
    for flags in gc.FLAGS:
        _, p, f = check_pick(ctx, sp, w, h, kind, big, None, None, BLOCKS, *args, "blocks alone", max_stale=big, flags=flags)
        assert 0 < p["n_stale"] < count and f["n_runs"] == 9 and f["merged"] == 0
    ns = min(p["n_stale"], big - 7)
    first = check_pick(ctx, sp, w, h, kind, ns + 7, None, None, BLOCKS, *args, "all of S and 7 picks", max_stale=ns + 7, flags=3)
    again = check_pick(ctx, sp, w, h, kind, ns + 7, None, None, BLOCKS, *args, "the same call twice", max_stale=ns + 7, flags=3)
    assert (first[0] == again[0]).all()
    for skip in (1, ns - 1, ns, ns + 5):
        check_pick(ctx, sp, w, h, kind, 70, None, None, BLOCKS, *args, "skip", max_stale=70, skip_stale=skip, cursor=9, flags=1)
    check_pick(ctx, sp, w, h, kind, 70, None, None, [5], *args, "max_stale < n", max_stale=30, cursor=2**40 + 3)
    # the caller's boxes and light cubes mixed in, with both depth flags, expand 0 and 2
    for flags, expand in ((0, 1), (3, 1), (2, 0), (1, 2)):
        check_pick(ctx, sp, w, h, kind, big, boxes, cubes, BLOCKS, *args, "boxes, cubes and blocks", max_stale=big, flags=flags, expand=expand)
    check_pick(ctx, sp, w, h, kind, 300, boxes, None, [5, 5], *args, "boxes and blocks", max_stale=200, skip_stale=17, flags=1)
    # merged: one box, the bounds; and a find of no capacity adds nothing
    _, p1, f1 = check_pick(ctx, sp, w, h, kind, big, None, cubes[:5], BLOCKS, *args, "merged", max_runs=8, max_stale=big, flags=3)
    assert f1["merged"] == 1 and f1["n_written"] == 1 and f1["n_runs"] == 9
    _, p0, f0 = check_pick(ctx, sp, w, h, kind, big, None, cubes[:5], BLOCKS, *args, "merged, no capacity", max_runs=0, max_stale=big, flags=3)
    assert f0["merged"] == 1 and f0["n_written"] == 0 and p0["n_stale"] < p1["n_stale"]
    _, _, f9 = check_pick(ctx, sp, w, h, kind, big, None, None, BLOCKS, *args, "capacity exactly n_runs", max_runs=9, max_stale=big)
    assert f9["merged"] == 0 and f9["n_written"] == 9
    # nothing is looked at: no find runs and found is zero; with no block the call is aic_pick_stale_cubes
    _, p, f = check_pick(ctx, sp, w, h, kind, 50, boxes, cubes, BLOCKS, *args, "max_stale = 0", cursor=4)
    assert f == ref.ZERO_INFO and p["n_from_order"] == 50 and p["n_stale"] == 0
    _, p, f = check_pick(ctx, sp, w, h, kind, 50, boxes, cubes, [], *args, "no blocks", max_stale=50, flags=3)
    assert f == ref.ZERO_INFO and p["n_stale"] > 0
    _, p, f = check_pick(ctx, sp, w, h, kind, 50, None, None, [], *args, "nothing at all", max_stale=50, flags=3, cursor=7)
    assert f == ref.ZERO_INFO and p["n_stale"] == 0 and p["next_cursor"] == 57
    check_pick(ctx, sp, w, h, kind, 50, None, None, BLOCKS, None, order_dev, frame, "NULL src without a depth flag", max_stale=50)
    assert (src.cpu().numpy() == src_bytes).all(), "src is only read"


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------

def load_case(ctx, name, antialiasing):
    """uploads space A of the redefinition; returns (the Split frame's description, view_projection)"""
    inv, vp, zw = B.camera(name)
    ctx.upload_space(WORLD, B.base(B.scene_of(name)))
    ctx.set_options(WORLD, to_abi_options(B.S.options(antialiasing)))
    ctx.clear_space(UI)
    ctx.set_depth_transform(zw)
    return ctx.make_frame(B.W, B.HT, world_inv=inv, flags=abi.FRAME_OUT_SPLIT), vp


def differing(a, b, count):
    return (a[:count * 8].view(np.uint64) != b[:count * 8].view(np.uint64)) | (a[count * 8:].view(np.uint32) != b[count * 8:].view(np.uint32))


@gpu
@pytest.mark.parametrize("antialiasing", B.ANTIALIASING)
@pytest.mark.parametrize("name", B.CASES)
def test_a_redefined_block_is_complete_after_tracing_the_stale_pixels(ctx, name, antialiasing):
    """A resident Split frame of A; aic_replace_blocks; every stale pixel of aic_pick_stale_blocks traced in place: the resident frame is a fresh Split
    render of B byte for byte, both planes, and the stale set is the restatement's, a part of the frame."""
    w, h = B.W, B.HT
    count = w * h
    try:
        f, vp = load_case(ctx, name, antialiasing)
        resident = rp.device_bytes(count * 12)
        ctx.render_submit(f, resident.data_ptr(), 0)
        ctx.render_wait(0)
        ctx.synchronize()
        before = resident.cpu().numpy().copy()
        ctx.replace_blocks(WORLD, [(B.block_of(name), B.new_block(name))])
        s = B.stale_set(name, 1)
        n_stale = int(s.sum())
        order = gs.picker_order(w, h)
        picks = pk.out_words(n_stale)
        info = ctx.pick_stale_blocks(vp, w, h, n_stale, None, None, WORLD, [B.block_of(name)], resident.data_ptr(), pk.to_device_words(order).data_ptr(), picks.data_ptr(),
                                     max_stale=n_stale)
        print(f"{name} aa {antialiasing}: {info.found.n_cubes} cubes in {info.found.n_runs} runs, n_stale {info.pick.n_stale} (restated {n_stale}) of {count}, "
              f"find {info.found.kernel_ms:.3f} ms, pick {info.pick.kernel_ms:.3f} ms")
        assert (info.pick.n_stale, info.pick.n_from_stale, info.pick.n_from_order, info.pick.whole_frame) == (n_stale, n_stale, 0, 0)
        assert info.found.n_runs == len(B.boxes(name)) == info.found.n_written and n_stale <= 0.4 * count
        listed = picks.cpu().numpy().view(np.uint32)[:n_stale]
        assert (listed == stale_ref.rank_list(s, order)).all()
        tinfo = ctx.trace_pixels_device(f, n_stale, picks.data_ptr(), resident.data_ptr(), in_place=True)
        assert tinfo.rows_rendered == n_stale
        after = resident.cpu().numpy()
        fresh = ctx.render(f)
        want = rp.frame_bytes(fresh["color_f16"].view(np.uint16), fresh["depth"])
        changed = differing(before, want, count)
        assert changed.sum() >= 1 and not (changed & ~s).any(), "the redefinition shows, and only inside S"
        assert (after == want).all()
    finally:
        ctx.set_depth_transform((1.0, 0.0, 0.0, 1.0))


@gpu
def test_host_mirror_refreshes_a_redefined_block_from_its_own_records():
    """HipRtRenderer: draw_split of terrace's A, the wall redefined through Space.set_block_data and a cube edited beside it, update(), then
    pick_stale_blocks() 100 picks a frame until no stale pixel is left, trace_pixels_into each list: the resident frame is draw_split of B byte for byte,
    with fewer stale pixels than the frame has -- changed_boxes() alone names the whole space."""
    import all_is_cubes_amd as A
    from all_is_cubes_amd import _host as H

    w, h = 40, 24
    n = w * h
    name = "terrace_alpha"
    sp = B.base(B.scene_of(name))
    eye, target = B.eye_target(name)
    cams = H.StandardCameras()
    cams.graphics_options = H.GraphicsOptions()
    cams.viewport = H.Viewport.with_scale(1.0, w, h)
    space = A.space_from_flat(sp)
    cams.world_space = space
    cams.world_view_transform = H.look_at_y_up(eye, target)
    r = H.HipRtRenderer(cams)
    r.update()
    assert r.changed_blocks() == [] and [list(b) for b in r.changed_cube_boxes()] == [[0, 0, 0, 8, 4, 8]] == [list(b) for b in r.changed_boxes()], "a whole upload"
    resident = rp.to_device(rp.split_bytes(r.draw_split()))
    before = resident.cpu().numpy().copy()
    r.update()
    assert r.changed_boxes() == [] and r.changed_blocks() == [] and r.changed_cube_boxes() == []
    space.set_block_data(B.block_of(name), A.evoxels_from_blockdef(B.new_block(name)))
    space.set(6, 1, 5, 0)  # the green cube goes
    r.update()
    assert r.changed_blocks() == [B.block_of(name)] and [list(b) for b in r.changed_cube_boxes()] == [[6, 1, 5, 7, 2, 6]] and r.pick_skip_stale == 0
    assert [list(b) for b in r.changed_boxes()] == [[0, 0, 0, 8, 4, 8]], "changed_boxes() is what it was"
    boxes, found = r.find_block_cubes([B.block_of(name)], 64)
    assert np.array(boxes, np.int32).tolist() == B.boxes(name).tolist() and found["n_cubes"] == 24 and found["merged"] == 0
    order = abi.pixel_order(w, h)[0]
    order_dev = pk.to_device_words(order)
    per_frame = 100
    listed = []
    for _ in range(n // per_frame + 2):
        picks = pk.out_words(per_frame)
        got = r.pick_stale_blocks(resident.data_ptr(), order_dev.data_ptr(), picks.data_ptr(), per_frame, per_frame)
        assert got["found"]["n_runs"] == len(B.boxes(name)) and got["pick"]["n_stale"] < n
        if got["pick"]["n_from_stale"] == 0:
            break
        listed.append(picks.cpu().numpy().view(np.uint32)[:got["pick"]["n_from_stale"]].copy())
        r.trace_pixels_into(resident.data_ptr(), picks.data_ptr(), got["pick"]["n_from_stale"])
    listed = np.concatenate(listed)
    assert r.pick_skip_stale == len(listed) == got["pick"]["n_stale"] and len(set(listed.tolist())) == len(listed)
    after = resident.cpu().numpy()
    want = rp.split_bytes(r.draw_split())
    assert (after == want).all()
    rest = np.ones(n, bool)
    rest[listed] = False
    assert not differing(after, before, n)[rest].any()
    assert (before != want).any(), "the redefinition shows"


@gpu
def test_beside_frames_in_flight_and_a_submitted_light_update(ctx):
    """both calls with a frame in flight on slot 1 and a light update submitted: the lists equal an idle twin's, the light update is still unpublished
    afterwards (aic_light_changed_count answers for the published volume), and the frame and the relit volume are what the twin arrives at"""
    name = "terrace_recolour"
    w, h = B.W, B.HT
    count = w * h
    twin = abi.Context(0)
    try:
        results = []
        for c, busy in ((twin, False), (ctx, True)):
            f, vp = load_case(c, name, 0)
            c.replace_blocks(WORLD, [(B.block_of(name), B.new_block(name))])
            c.update_cubes(WORLD, [(1, 2, 1)], [0])  # the red cube goes: the relight changes texels around it
            c.light_cubes_changed(WORLD, [(1, 2, 1)])
            frame_out = rp.device_bytes(count * 12)
            if busy:
                c.render_submit(f, frame_out.data_ptr(), 1)
                c.evaluate_light_submit(WORLD, 8, fast=False, queue=[])
                stored = c.light_changed(WORLD, take=False)[0]  # what aic_light_cubes_changed stored at once; the update's changes join when it is published
            boxes, found = c.find_block_cubes(WORLD, [B.block_of(name)], 64)
            picks = pk.out_words(count)
            info = c.pick_stale_blocks(vp, w, h, count, None, None, WORLD, [B.block_of(name)], 0, 0, picks.data_ptr(), max_stale=count)
            if busy:
                while not c.evaluate_light_done(WORLD):
                    pass
                assert c.light_changed(WORLD, take=False)[0] == stored, "neither call ended the update: finished, it is still not published"
                finfo = c.render_wait(1)
                linfo = c.evaluate_light_wait(WORLD)
                assert finfo.rows_rendered == h and linfo.updates > 0 and c.light_changed(WORLD, take=False)[0] > stored, "the wait published it"
            else:
                c.render_submit(f, frame_out.data_ptr(), 1)
                c.render_wait(1)
                c.evaluate_light(WORLD, 8, fast=False, queue=[])
            c.synchronize()
            results.append((boxes.tobytes(), found_dict(found), picks.cpu().numpy().tobytes(), gc.info_dict(info.pick), found_dict(info.found), frame_out.cpu().numpy().tobytes(),
                            c.read_light_volume(WORLD, B.base(B.scene_of(name)).size).tobytes()))
        assert results[0][1]["n_runs"] == 8 and results[0][3]["n_stale"] == int(B.stale_set(name, 1).sum())
        for k, (a, b) in enumerate(zip(*results)):
            assert a == b, k
    finally:
        twin.close()
        ctx.set_depth_transform((1.0, 0.0, 0.0, 1.0))


@gpu
def test_rejections_leave_the_context_usable(ctx):
    import torch

    w, h = 61, 37
    sp = B.base(SCENE)
    ctx.upload_space(WORLD, sp)
    ctx.clear_space(UI)
    frame = gc.frame(w, h)
    src_bytes = rp.frame_bytes(*frame)
    src = rp.to_device(src_bytes)
    order_dev = pk.to_device_words(gs.picker_order(w, h))
    boxes, cubes = gc.cube_set("257")
    vp = gc.view_projection(w, h)
    n = 40
    out = pk.out_words(n + 4)
    box_out = np.full((16, 6), 0x5A5A5A5A, np.int32)
    idx = np.array(BLOCKS, np.uint32)
    bad_idx = np.array([5, len(sp.blocks)], np.uint32)

    def good(what):
        check_pick(ctx, sp, w, h, "picker", n, boxes, cubes, BLOCKS, src, order_dev, frame, what, max_stale=n, skip_stale=1, cursor=9, flags=3)
        check_find(ctx, sp, BLOCKS, 16, what)

    def rejected(fn, what):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, what
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all(), what
        assert (src.cpu().numpy() == src_bytes).all() and (box_out == 0x5A5A5A5A).all(), what
        good(what)

    def desc(n=n, layer=WORLD, blocks=idx, n_blocks=None, max_runs=64, width=w, n_boxes=None, flags=3, expand=1):
        d = abi.StaleBlocksDesc()
        d.cubes.width, d.cubes.height, d.cubes.n, d.cubes.max_stale, d.cubes.flags, d.cubes.expand = width, h, n, n, flags, expand
        d.cubes.view_projection = (C.c_double * 16)(*vp)
        d.cubes.n_boxes = len(boxes) if n_boxes is None else n_boxes
        d.cubes.n_light_cubes = len(cubes)
        d.cubes.boxes, d.cubes.light_cubes = boxes.ctypes.data, cubes.ctypes.data
        d.layer, d.max_runs = layer, max_runs
        d.n_blocks = (len(blocks) if blocks is not None else 0) if n_blocks is None else n_blocks
        d.block_indices = blocks.ctypes.data if blocks is not None else None
        return d

    info = abi.StaleBlocksInfo()
    finfo = abi.BlockCubesInfo()

    def raw_pick(d, src_ptr=-1, out_ptr=-1, info_ptr=-1):
        ptr = lambda v, default: default if v == -1 else v
        ctx._check(ctx._lib.aic_pick_stale_blocks(ctx._h, None if d is None else C.byref(d), C.c_void_p(ptr(src_ptr, src.data_ptr())), C.c_void_p(order_dev.data_ptr()),
                                                  C.c_void_p(ptr(out_ptr, out.data_ptr())), ptr(info_ptr, C.byref(info))))

    def raw_find(layer=WORLD, blocks=idx, n_blocks=None, capacity=16, dst=-1, info_ptr=-1):
        ctx._check(ctx._lib.aic_find_block_cubes(ctx._h, layer, (len(blocks) if blocks is not None else 0) if n_blocks is None else n_blocks,
                                                 C.c_void_p(blocks.ctypes.data if blocks is not None else None), capacity,
                                                 C.c_void_p(box_out.ctypes.data if dst == -1 else dst), C.byref(finfo) if info_ptr == -1 else info_ptr))

    good("before")
    # what the find adds
    rejected(lambda: raw_pick(desc(), info_ptr=None), "NULL info")
    rejected(lambda: raw_find(info_ptr=None), "NULL info, find")
    rejected(lambda: raw_pick(desc(blocks=None, n_blocks=2)), "NULL indices")
    rejected(lambda: raw_find(blocks=None, n_blocks=2), "NULL indices, find")
    rejected(lambda: raw_pick(desc(blocks=bad_idx)), "an index at the block count")
    rejected(lambda: raw_find(blocks=bad_idx), "an index at the block count, find")
    for layer in (2, -1, UI):  # (no UI space is uploaded)
        rejected(lambda: raw_pick(desc(layer=layer)), f"layer {layer}")
        rejected(lambda: raw_find(layer=layer), f"layer {layer}, find")
    rejected(lambda: raw_find(dst=None), "NULL out_boxes with a capacity")
    rejected(lambda: raw_pick(desc(max_runs=2**32 - 1 - len(boxes) - len(cubes) + 1)), "boxes + max_runs + light cubes above 2^32 - 1")
    # everything aic_pick_stale_cubes rejects, through the same checks: one of each kind
    rejected(lambda: raw_pick(None), "NULL desc")
    rejected(lambda: raw_pick(desc(), out_ptr=None), "NULL pixels_out")
    rejected(lambda: raw_pick(desc(), out_ptr=out.data_ptr() + 2), "misaligned pixels_out")
    rejected(lambda: raw_pick(desc(), src_ptr=src.data_ptr() + 4), "misaligned src")
    rejected(lambda: raw_pick(desc(), src_ptr=None), "NULL src with a depth flag")
    rejected(lambda: raw_pick(desc(width=65536)), "width above 65535")
    rejected(lambda: raw_pick(desc(flags=4)), "unknown flag bits")
    rejected(lambda: raw_pick(desc(expand=-1)), "a negative expand")
    rejected(lambda: raw_pick(desc(n=2048 * 65535 + 1)), "too many picks")
    # a frame still occupying slot 0
    ctx.set_options(WORLD, abi.make_options())
    import oracle

    eye = (4.3, 4.0, 10.0)
    _, _, inv = oracle.camera_matrices(90.0, 200.0, 40 / 24, oracle.look_at_y_up(eye, (4.0, 1.0, 4.0)), eye)
    busy = rp.device_bytes(40 * 24 * 4)
    ctx.render_submit(ctx.make_frame(40, 24, world_inv=inv), busy.data_ptr(), 0)
    for fn in (lambda: raw_pick(desc()), lambda: raw_find()):
        with pytest.raises(abi.AicError) as err:
            fn()
        assert err.value.code == AIC_ERR_INVALID, "slot 0 busy"
    ctx.render_wait(0)
    ctx.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL_WORD).all() and (box_out == 0x5A5A5A5A).all()
    good("after slot 0 busy")
    # legal: the last value that fits, a find of no capacity without boxes to write to, no blocks with NULL indices
    raw_pick(desc(max_runs=2**32 - 1 - len(boxes) - len(cubes)))
    assert info.found.merged == 0 and info.found.n_written == 9
    raw_find(capacity=0, dst=None)
    assert finfo.merged == 1 and finfo.n_written == 0 and finfo.n_runs == 9
    raw_find(blocks=None, n_blocks=0, capacity=0, dst=None)
    assert bytes(finfo) == bytes(C.sizeof(finfo))
    # n = 0: AIC_OK, nothing written, the info zeroed
    C.memset(C.byref(info), 0xFF, C.sizeof(info))
    raw_pick(desc(n=0), out_ptr=None, src_ptr=None)
    assert bytes(info) == bytes(C.sizeof(info))
    good("after the legal calls")
    torch.cuda.synchronize()
