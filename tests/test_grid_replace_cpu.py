"""aic_replace_cube_grid without a device: tests/grid_replace_ref.py against the definition written as loops, the run rule on hand-made arrays, the
argument checks of all_is_cubes_amd/abi.py on CPU tensors, and the dump record's round trip through all_is_cubes_amd/replay.py."""
import numpy as np
import pytest

from all_is_cubes_amd import abi, flat, replay
from tests import grid_replace_ref as ref


def report_by_loops(lo, old, new, capacity):
    """The header's text, one cube at a time."""
    sx, sy, sz = old.shape
    runs, n_cubes = [], 0
    lows, highs = [None] * 3, [None] * 3
    for x in range(sx):
        for y in range(sy):
            z = 0
            while z < sz:
                if int(old[x, y, z]) == int(new[x, y, z]):
                    z += 1
                    continue
                z0 = z
                while z < sz and int(old[x, y, z]) != int(new[x, y, z]):
                    z += 1
                runs.append([lo[0] + x, lo[1] + y, lo[2] + z0, lo[0] + x + 1, lo[1] + y + 1, lo[2] + z])
                n_cubes += z - z0
                for a, (p, q) in enumerate(((x, x + 1), (y, y + 1), (z0, z))):
                    lows[a] = p if lows[a] is None else min(lows[a], p)
                    highs[a] = q if highs[a] is None else max(highs[a], q)
    if not runs:
        return np.zeros((0, 6), np.int32), dict(ref.ZERO_INFO)
    bounds = [lo[a] + lows[a] for a in range(3)] + [lo[a] + highs[a] for a in range(3)]
    merged = len(runs) > capacity
    written = ([bounds] if capacity >= 1 else []) if merged else runs
    return (np.array(written, np.int32).reshape(-1, 6),
            {"n_cubes": n_cubes, "n_runs": len(runs), "bounds": bounds, "n_written": len(written), "merged": int(merged)})


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 3), (2, 5, 5), (3, 3, 40), (2, 3, 17)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("share", [0.0, 0.01, 0.5, 0.99, 1.0])
def test_the_restatement_is_the_definition(shape, share):
    rng = np.random.default_rng(hash((shape, share)) % 2**32)
    lo = (-7, 3, -20)
    old = rng.integers(0, 5, shape).astype(np.uint16)
    new = old.copy()
    pick = rng.random(shape) < share
    new[pick] = (old[pick] + rng.integers(1, 5, int(pick.sum()))) % 5
    assert (ref.changed(old, new) == pick).all()
    n_runs = len(report_by_loops(lo, old, new, 1 << 30)[0])
    for capacity in {0, 1, max(n_runs - 1, 0), n_runs, n_runs + 1}:
        got, want = ref.report(lo, old, new, capacity), report_by_loops(lo, old, new, capacity)
        assert got[1] == want[1], capacity
        assert got[0].dtype == np.int32 and got[0].tolist() == want[0].tolist(), capacity


def test_a_run_ends_with_its_row():
    old = np.zeros((1, 2, 4), np.uint16)
    new = old.copy()
    new[0, 0, 2:] = 1  # ... to z = sz - 1
    new[0, 1, 0] = 1   # z = 0 of the next row: adjacent in memory
    boxes, info = ref.report((10, 20, 30), old, new, 8)
    assert boxes.tolist() == [[10, 20, 32, 11, 21, 34], [10, 21, 30, 11, 22, 31]]
    assert info == {"n_cubes": 3, "n_runs": 2, "bounds": [10, 20, 30, 11, 22, 34], "n_written": 2, "merged": 0}


def test_nothing_changed_is_a_zero_info_and_tags_never_count():
    old = np.arange(24, dtype=np.uint16).reshape(2, 3, 4)
    for capacity in (0, 1, 100):
        boxes, info = ref.report((0, 0, 0), old, old.copy(), capacity)
        assert boxes.shape == (0, 6) and info == ref.ZERO_INFO
    assert info == {"n_cubes": 0, "n_runs": 0, "bounds": [0] * 6, "n_written": 0, "merged": 0}


def test_the_capacity_table():
    old = np.zeros((2, 2, 5), np.uint16)
    new = old.copy()
    new[0, 0, 1] = new[0, 0, 3] = new[1, 1, 4] = 2  # three runs
    bounds = [0, 0, 1, 2, 2, 5]
    rows = {3: (3, 0), 4: (3, 0), 2: (1, 1), 1: (1, 1), 0: (0, 1)}
    for capacity, (n_written, merged) in rows.items():
        boxes, info = ref.report((0, 0, 0), old, new, capacity)
        assert (info["n_runs"], info["n_cubes"], info["bounds"]) == (3, 3, bounds)
        assert (info["n_written"], info["merged"], len(boxes)) == (n_written, merged, n_written), capacity
        if merged and capacity:
            assert boxes.tolist() == [bounds]
    boxes, info = ref.report((0, 0, 0), old, old, 0)  # n_runs = 0
    assert (info["n_written"], info["merged"]) == (0, 0)


def test_replace_applies_to_the_model_and_refuses_an_index_out_of_range():
    sp = flat.FlatSpace((1, 2, 3), (2, 2, 3))
    sp.add_block(flat.air())
    sp.add_block(flat.atom((0.5, 0.5, 0.5, 1.0)))
    new = np.zeros(sp.size, np.uint16)
    new[1, 1, 2] = 1
    boxes, info = ref.replace(sp, new, 4)
    assert boxes.tolist() == [[2, 3, 5, 3, 4, 6]] and info["n_cubes"] == 1 and (sp.block_index == new).all()
    bad = new.copy()
    bad[0, 0, 0] = 2
    with pytest.raises(ValueError):
        ref.replace(sp, bad, 4)
    assert (sp.block_index == new).all()
    assert (ref.grid_after(sp) >> 14).max() == 2  # class + 1 of the visible atom


# --- abi.py's checks, on tensors that never reach a device --------------------------------------------------------------------------------
def test_argument_checks_on_cpu_tensors():
    import torch

    n = 24
    check = abi.device_array_ptr
    good = torch.zeros(n, dtype=torch.int16)
    with pytest.raises(ValueError, match="dtype"):
        check(torch.zeros(n, dtype=torch.int32), ("uint16", "int16"), n, "block_index", 0)
    with pytest.raises(ValueError, match="dtype"):
        check(torch.zeros(n, dtype=torch.float16), ("uint16", "int16"), n, "block_index", 0)
    with pytest.raises(ValueError, match="elements"):
        check(torch.zeros(n + 1, dtype=torch.int16), ("uint16", "int16"), n, "block_index", 0)
    with pytest.raises(ValueError, match="contiguous"):
        check(torch.zeros(2 * n, dtype=torch.int16)[::2], ("uint16", "int16"), n, "block_index", 0)
    with pytest.raises(ValueError, match="not in device memory"):
        check(good, ("uint16", "int16"), n, "block_index", 0)
    with pytest.raises(ValueError, match="not in device memory"):
        check(torch.zeros(4 * n, dtype=torch.uint8), ("uint8",), 4 * n, "light", 0)
    with pytest.raises(TypeError):
        check(np.zeros(n, np.uint16), ("uint16", "int16"), n, "block_index", 0)
    assert check(None, ("uint8",), 4 * n, "light", 0) == 0
    assert check(0x7F0000001000, ("uint16", "int16"), n, "block_index", 0) == 0x7F0000001000  # a raw pointer passes as it is


def test_the_three_calls_have_signatures():
    lib = abi.load()
    assert len(lib.aic_replace_cube_grid.argtypes) == 7 and len(lib.aic_copy_cube_grid.argtypes) == 4 and len(lib.aic_update_light_volume_device.argtypes) == 3
    for name in ("replace_cube_grid", "copy_cube_grid", "update_light_volume_device"):
        assert callable(getattr(abi.Context, name))


# --- the dump record ----------------------------------------------------------------------------------------------------------------------
def test_the_dump_record_round_trips(tmp_path):
    sp = flat.FlatSpace((-1, 0, 2), (2, 3, 5))
    sp.add_block(flat.air())
    sp.add_block(flat.atom((0.9, 0.1, 0.1, 1.0)))
    rng = np.random.default_rng(3)
    new = rng.integers(0, 2, sp.size).astype(np.uint16)
    light = rng.integers(0, 255, sp.size + (4,)).astype(np.uint8)
    path = tmp_path / "grid.dump"
    with replay.DumpWriter(path) as w:
        w.upload_space(0, sp)
        w.replace_cube_grid(0, new, None, capacity=7)
        w.replace_cube_grid(0, new[::-1].copy(), light, capacity=0)
    records = list(replay.read_dump(path))
    assert [r.tag for r in records] == [replay.UPLOAD, replay.GRID, replay.GRID] and replay.GRID == 8
    a, b = records[1].data, records[2].data
    assert a["capacity"] == 7 and a["light"] is None and (a["block_index"] == new.reshape(-1)).all() and a["block_index"].dtype == np.uint16
    assert b["capacity"] == 0 and (b["light"] == light.reshape(-1, 4)).all() and (b["block_index"] == new[::-1].reshape(-1)).all()
    state = replay.SceneState()
    state.apply(records[0])
    state.apply(records[1])
    assert (state.spaces[0].block_index == new).all() and (state.spaces[0].light == sp.light).all()
    state.apply(records[2])
    assert (state.spaces[0].block_index == new[::-1]).all() and (state.spaces[0].light == light).all()
    # the layout the library writes: {u64 n, u32 has_light, u32 capacity}, the indices, the light
    blob = path.read_bytes()
    n = new.size
    tail = blob[-(16 + 16 + 2 * n + 4 * n):]
    assert np.frombuffer(tail[:16], "<u4").tolist()[:2] == [replay.GRID, 0] and int(np.frombuffer(tail[8:16], "<u8")[0]) == 16 + 6 * n
    assert int(np.frombuffer(tail[16:24], "<u8")[0]) == n and np.frombuffer(tail[24:32], "<u4").tolist() == [1, 0]
