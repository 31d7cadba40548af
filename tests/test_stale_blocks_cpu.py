"""CPU tests of the stale set of a re-evaluated block: the restatement against the rule written as plain loops, the rule's
conservativeness against the oracle -- every pixel outside the rectangles of the cubes that hold the block is byte-identical before and after the block's
definition changed --, the struct layouts as a C compiler reads the header, and the names across the layers. No device is needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from all_is_cubes_amd import abi, flat
from tests import stale_block_scenes as B
from tests import stale_blocks_ref as ref
from tests.test_stale_cpu import frames_differ

ROOT = Path(__file__).resolve().parent.parent
COUNT = B.W * B.HT
# 1x3x683: 2049 entries, one past a workgroup's 2048; 4x4x8: a row is a lane's group of 8 entries; 1x2x5000: a row longer than a workgroup's entries, so
# that under "all" a workgroup lies wholly inside one run and holds matches but neither a start nor an end
GRIDS = [(1, 1, 1), (3, 3, 40), (2, 5, 51), (4, 4, 8), (2, 2, 64), (1, 3, 683), (5, 7, 300), (1, 2, 5000)]
PATTERNS = ["none", "one", "every_other", "all", "random"]
LO = (-7, 3, -2**20)


def grid_space(size, pattern, lo=LO):
    """a space of `size` whose cubes hold block 1 (matching), 2 or 0 by `pattern`; (space, the indices to look for)"""
    n = int(np.prod(size))
    rng = np.random.default_rng(n)
    flat_index = np.zeros(n, np.uint16)
    if pattern == "one":
        flat_index[n // 2] = 1
    elif pattern == "every_other":
        flat_index[::2] = 1
        flat_index[1::2] = 2
    elif pattern == "all":
        flat_index[:] = 1
    elif pattern == "random":  # runs of random lengths, which cross rows, lanes' groups and entry 2048
        at = 0
        while at < n:
            length = int(rng.integers(1, 20))
            flat_index[at:at + length] = int(rng.integers(0, 3))
            at += length
    sp = flat.FlatSpace(lo, size, block_index=flat_index.reshape(size))
    for b in (flat.air(), flat.atom((0.9, 0.1, 0.1, 1.0)), flat.atom((0.1, 0.8, 0.2, 1.0))):
        sp.add_block(b)
    return sp, [1]


def by_loops(sp, indices, capacity):
    """the definition, entry by entry in linear order"""
    sx, sy, sz = (int(v) for v in sp.size)
    wanted = set(int(i) for i in indices)
    runs, n_cubes, lo, hi = [], 0, [None] * 3, [None] * 3
    for x in range(sx):
        for y in range(sy):
            z = 0
            while z < sz:
                if int(sp.block_index[x, y, z]) not in wanted:
                    z += 1
                    continue
                z0 = z
                while z < sz and int(sp.block_index[x, y, z]) in wanted:
                    z += 1
                runs.append([sp.lo[0] + x, sp.lo[1] + y, sp.lo[2] + z0, sp.lo[0] + x + 1, sp.lo[1] + y + 1, sp.lo[2] + z])
                n_cubes += z - z0
                for a, (l, h) in enumerate([(x, x + 1), (y, y + 1), (z0, z)]):
                    lo[a] = l if lo[a] is None else min(lo[a], l)
                    hi[a] = h if hi[a] is None else max(hi[a], h)
    bounds = [sp.lo[a] + lo[a] for a in range(3)] + [sp.lo[a] + hi[a] for a in range(3)] if runs else [0] * 6
    merged = len(runs) > capacity
    written = ([bounds] if capacity >= 1 else []) if merged else runs
    return written, {"n_cubes": n_cubes, "n_runs": len(runs), "bounds": bounds, "n_written": len(written), "merged": int(merged)}


@pytest.mark.parametrize("size", GRIDS)
def test_the_restatement_is_the_definition_in_plain_loops(size):
    for pattern in PATTERNS:
        for lo in (LO, (0, 0, 0)):
            sp, indices = grid_space(size, pattern, lo)
            n_runs = ref.find(sp, indices, 1 << 30)[1]["n_runs"]
            for capacity in sorted({1 << 30, n_runs, max(n_runs - 1, 0), 0}):
                got, info = ref.find(sp, indices, capacity)
                want, want_info = by_loops(sp, indices, capacity)
                assert info == want_info, (size, pattern, capacity)
                assert got.dtype == np.int32 and got.tolist() == want, (size, pattern, capacity)
            # duplicates, and a second index
            assert ref.find(sp, [1, 1, 1], 1 << 30)[0].tolist() == ref.find(sp, [1], 1 << 30)[0].tolist()
            got, info = ref.find(sp, [2, 1], 1 << 30)
            want, want_info = by_loops(sp, [1, 2], 1 << 30)
            assert got.tolist() == want and info == want_info
    n = int(np.prod(size))
    assert ref.find(grid_space(size, "all")[0], [1], n)[1]["n_runs"] == size[0] * size[1]
    assert ref.find(grid_space(size, "none")[0], [1], n) [1] == ref.ZERO_INFO


def test_matches_at_the_end_of_a_row_and_the_start_of_the_next_do_not_merge():
    sp = flat.FlatSpace((0, 0, 0), (2, 2, 5))
    for b in (flat.air(), flat.atom((1.0, 0.0, 0.0, 1.0))):
        sp.add_block(b)
    for cube in [(0, 0, 4), (0, 1, 0), (0, 1, 4), (1, 0, 0)]:  # linear neighbours 4|5 and 9|10
        sp.set(cube, 1)
    got, info = ref.find(sp, [1], 8)
    assert got.tolist() == [[0, 0, 4, 1, 1, 5], [0, 1, 0, 1, 2, 1], [0, 1, 4, 1, 2, 5], [1, 0, 0, 2, 1, 1]]
    assert info == {"n_cubes": 4, "n_runs": 4, "bounds": [0, 0, 0, 2, 2, 5], "n_written": 4, "merged": 0}
    assert ref.find(sp, [1], 3) [0].tolist() == [[0, 0, 0, 2, 2, 5]] and ref.find(sp, [1], 3)[1]["merged"] == 1
    assert len(ref.find(sp, [1], 0)[0]) == 0 and ref.find(sp, [1], 0)[1]["merged"] == 1


@pytest.mark.parametrize("antialiasing", B.ANTIALIASING)
@pytest.mark.parametrize("name", B.CASES)
def test_pixels_outside_the_stale_set_do_not_change_when_a_block_is_redefined(name, antialiasing):
    """A against B, the same grid and light volume with one block redefined: no pixel outside the rectangles of the cubes that hold the block changes,
    with expand 0 and with expand 1; at least one pixel inside does; and the set is at most 40 % of the frame, so marking everything cannot pass."""
    differ = frames_differ(B.oracle_split(name, "A", antialiasing), B.oracle_split(name, "B", antialiasing))
    s0, s1 = B.stale_set(name, 0), B.stale_set(name, 1)
    print(f"{name} aa {antialiasing}: {len(B.boxes(name))} runs, {int(differ.sum())} pixels differ, S expand 0 {int(s0.sum())} ({100 * s0.sum() / COUNT:.1f} %), "
          f"expand 1 {int(s1.sum())} ({100 * s1.sum() / COUNT:.1f} %) of {COUNT}")
    assert differ.sum() >= 1, "the redefinition shows"
    assert not (differ & ~s0).any()
    assert not (differ & ~s1).any()
    assert not (s0 & ~s1).any()
    assert s1.sum() <= 0.40 * COUNT


def test_the_ghost_block_is_invisible_and_sits_in_open_cubes_and_on_the_rim():
    from tests import cube_tags_ref as tags

    sp = B.base("ghost")
    assert tags.block_class(sp.blocks[B.GHOST]) == 0 and not sp.blocks[B.GHOST].is_air, "an invisible single voxel that is not AIR"
    held = sp.block_index == B.GHOST
    assert held.sum() == len(B.GHOST_CUBES)
    is_open = tags.open_cubes(sp)
    assert (held & is_open).sum() >= 2 and (held & ~is_open).sum() >= 2, "OPEN-tagged cubes (tag 0) and INVISIBLE-tagged ones"
    rim = np.ones(sp.size, bool)
    rim[1:-1, 1:-1, 1:-1] = False
    assert (held & rim).sum() >= 2


def test_structs_match_the_header():
    """sizeof and offsetof as a C compiler reads include/aic_hip.h, against the ctypes mirrors"""
    structs = {"aic_block_cubes_info": abi.BlockCubesInfo, "aic_stale_blocks_desc": abi.StaleBlocksDesc, "aic_stale_blocks_info": abi.StaleBlocksInfo,
               "aic_stale_cubes_desc": abi.StaleCubesDesc, "aic_stale_cubes_info": abi.StaleCubesInfo}
    fields = {name: [f[0] for f in t._fields_] for name, t in structs.items()}
    prints = "".join(f'printf("{name} %zu", sizeof({name}));' + "".join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields[name]) + 'printf("\\n");'
                     for name in structs)
    d = tempfile.mkdtemp(prefix="aic_stale_blocks_structs_")
    src = os.path.join(d, "s.c")
    Path(src).write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "aic_hip.h"\nint main(void) {{ {prints} return 0; }}\n')
    subprocess.run(["cc", "-I", str(ROOT / "include"), src, "-o", os.path.join(d, "s")], check=True)
    out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out if line}
    for name, t in structs.items():
        assert seen[name] == [C.sizeof(t)] + [getattr(t, f).offset for f in fields[name]], name
    assert seen["aic_block_cubes_info"] == [56, 0, 8, 16, 40, 44, 48, 52]
    assert seen["aic_stale_blocks_desc"] == [216, 0, 192, 196, 200, 208, 212] and seen["aic_stale_blocks_info"] == [96, 0, 40]
    assert (C.sizeof(abi.StaleCubesDesc), C.sizeof(abi.StaleCubesInfo)) == (192, 40), "no existing struct changed"


def test_names_agree_across_the_layers():
    lib = abi.load()
    arity = {"aic_find_block_cubes": 7, "aic_pick_stale_blocks": 6}
    header = (ROOT / "include" / "aic_hip.h").read_text()
    ffi = (ROOT / "rust" / "all-is-cubes-hip" / "src" / "ffi.rs").read_text()
    shim = (ROOT / "rust" / "all-is-cubes-hip" / "src" / "lib.rs").read_text()
    for name, n_args in arity.items():
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None and len(argtypes) == n_args and argtypes[0] is C.c_void_p, name
        assert re.search(rf"\bint {name}\(aic_ctx \*ctx,", header) and f"pub fn {name}(" in ffi and f"ffi::{name}(" in shim, name
    assert lib.aic_pick_stale_blocks.argtypes[1]._type_ is abi.StaleBlocksDesc and lib.aic_pick_stale_blocks.argtypes[5]._type_ is abi.StaleBlocksInfo
    assert lib.aic_find_block_cubes.argtypes[6]._type_ is abi.BlockCubesInfo
    for name in ("aic_block_cubes_info", "aic_stale_blocks_desc", "aic_stale_blocks_info"):
        assert f"typedef struct {name} {{" in header and f"pub struct {name} {{" in ffi, name
    for name in ("find_block_cubes", "pick_stale_blocks"):
        assert callable(getattr(abi.Context, name)) and f"fn {name}(" in shim, name
    from all_is_cubes_amd import _host as H

    for name in ("find_block_cubes", "pick_stale_blocks", "changed_blocks", "changed_cube_boxes", "changed_boxes"):
        assert hasattr(H.HipRtRenderer, name), name
    assert "pub fn changed_blocks(" in shim
    assert lib.aic_abi_version() == 3
