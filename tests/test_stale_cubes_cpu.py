"""CPU tests of the stale set of a light update: the rule's conservativeness against the oracle -- every pixel outside the stale set is
byte-identical under the old and the relit light volume --, the behind test's worth, the struct layouts as a C compiler reads the header, and the
binding. No device is needed."""
import ctypes as C
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from all_is_cubes_amd import abi
from tests import stale_cubes_ref as ref
from tests import stale_light_scenes as L
from tests import stale_ref
from tests.test_stale_cpu import frames_differ

ROOT = Path(__file__).resolve().parent.parent
COUNT = L.W * L.HT
# (light cubes that differ, pixels that differ None / Always, S by rectangles alone, S with the behind test None / Always, S with both tests None):
# found with the restatement over the oracle, and asserted as found
FOUND = {
    "plaza": (24, (646, 684), 4272, (1699, 1762), 1699),
    "terrace": (23, (293, 334), 1659, (753, 785), 743),
    "behind_wall": (22, (479, 493), 3434, (1460, 1469), 1412),
    "plaza_glass": (29, (818, 866), 4482, (1737, 1804), None),
}
UNION_FOUND = {"plaza": ((672, 714), (2257, 2305)), "terrace": ((308, 352), (1177, 1182)), "behind_wall": ((590, 603), (2699, 2699)),
               "plaza_glass": ((832, 880), (2257, 2305))}


@pytest.mark.parametrize("antialiasing", L.ANTIALIASING)
@pytest.mark.parametrize("name", L.CASES)
def test_pixels_outside_the_stale_set_do_not_change_under_a_relight(name, antialiasing):
    """B's blocks under A's light volume and under the volume the updater arrives at: every pixel outside S holds the same bytes in both frames -- by
    rectangles alone, with the behind test, and (opaque scenes, no antialiasing: the front test's domain) with both tests. The behind test leaves at most
    a third of the frame, so marking everything cannot pass, and is a proper subset of the plain set."""
    n_cubes, n_differ, n_plain, n_behind, n_both = FOUND[name]
    k = L.ANTIALIASING.index(antialiasing)
    cubes = L.relit(name)[1]
    differ = frames_differ(L.frame(name, "B", antialiasing), L.frame(name, "B'", antialiasing))
    plain, rects = L.stale_set(name, antialiasing, 0)
    behind, _ = L.stale_set(name, antialiasing, ref.DEPTH_BEHIND)
    print(f"{name} aa {antialiasing}: {len(cubes)} light cubes differ, {int(differ.sum())} pixels differ, S plain {int(plain.sum())}, behind {int(behind.sum())} of {COUNT}")
    assert len(cubes) >= 20 and differ.sum() >= 20, "the relight shows"
    assert not (differ & ~plain).any()
    assert not (differ & ~behind).any()
    assert behind.sum() <= COUNT // 3
    assert not (behind & ~plain).any() and behind.sum() < plain.sum()
    assert (stale_ref.rank_list(behind, None) == np.flatnonzero(behind)).all()
    assert np.isfinite(rects["dmax"]).all() and (rects["dmin"] < rects["dmax"]).all()
    if name == "plaza_glass":
        # (the sky is drawn behind everything: alpha is 1 throughout, and only the depth plane -- the glass's own -- tells a pane from what it covers)
        shows = frames_differ(L.frame(name, "B", antialiasing), L.frame("plaza", "B", antialiasing))
        assert shows.sum() >= 200 and (differ & shows).sum() >= 20, "glass in front of and behind changed light"
    if name in L.OPAQUE_CASES and antialiasing == 0:
        both, _ = L.stale_set(name, antialiasing, ref.DEPTH_BEHIND | ref.DEPTH_TEST)
        assert (L.frame(name, "B", antialiasing)[0][..., 3].view(np.float16) == 1.0).all(), "opaque only"
        assert not (differ & ~both).any() and not (both & ~behind).any()
        assert both.sum() == n_both
    assert (len(cubes), int(differ.sum()), int(plain.sum()), int(behind.sum())) == (n_cubes, n_differ[k], n_plain, n_behind[k])


@pytest.mark.parametrize("antialiasing", L.ANTIALIASING)
@pytest.mark.parametrize("name", L.CASES)
def test_edits_and_relight_together(name, antialiasing):
    """The resident frame of A against the frame of B': boxes = the edits (expand = 1), light cubes = the diff. Nothing outside S differs, without a
    depth flag and with the behind test read from the resident frame A."""
    k = L.ANTIALIASING.index(antialiasing)
    differ = frames_differ(L.frame(name, "A", antialiasing), L.frame(name, "B'", antialiasing))
    plain, rects = L.stale_set(name, antialiasing, 0, True)
    behind, _ = L.stale_set(name, antialiasing, ref.DEPTH_BEHIND, True)
    n_boxes = len(L.boxes(name))
    host = stale_ref.rects(L.S.camera(L.base(name))[1], L.W, L.HT, L.boxes(name), 1)
    for f in ("x0", "y0", "x1", "y1"):
        assert (rects[f][:n_boxes] == host[f]).all()
    assert rects["dmin"][:n_boxes].tobytes() == host["dmin"].tobytes(), "a box's rectangle is aic_stale_rects' own"
    print(f"{name} aa {antialiasing}: {int(differ.sum())} pixels differ, S plain {int(plain.sum())}, behind {int(behind.sum())}")
    assert not (differ & ~plain).any() and not (differ & ~behind).any() and not (behind & ~plain).any()
    assert (int(differ.sum()), int(behind.sum())) == (UNION_FOUND[name][0][k], UNION_FOUND[name][1][k])


def test_rectangles_of_boxes_are_the_host_helpers():
    """the first five fields against tests/stale_ref.py and aic_stale_rects over test_stale_cpu's cameras and boxes; dmax is never below dmin"""
    from tests import test_stale_cpu as sc

    rng = np.random.default_rng(3)
    for w, h in [(61, 37), (96, 64)]:
        for vp, eye, target in [sc.perspective(rng, w, h) for _ in range(4)] + [(sc.orthographic(), (3.0, 2.0, -10.0), (3.0, 2.0, 0.0))]:
            b = sc.boxes_around(rng, eye, target)
            for expand in (0, 1, 3):
                got, host = ref.rects(vp, w, h, b, (), expand), abi.stale_rects(vp, w, h, b, expand)
                for f in ("x0", "y0", "x1", "y1"):
                    assert (got[f] == host[f]).all()
                assert got["dmin"].tobytes() == host["dmin"].tobytes()
                full = got["x1"] > 0
                assert (got["dmax"][full] >= got["dmin"][full]).all() and (got["dmax"][~full] == 0).all()
                assert ((got["dmin"] == -np.inf) == (got["dmax"] == np.inf)).all()
    # a light cube is the box [q, q + 1) grown by one, whatever `expand` says
    vp = sc.orthographic()
    assert ref.rects(vp, 96, 64, (), [[3, 2, 0]], 5).tobytes() == ref.rects(vp, 96, 64, [[3, 2, 0, 4, 3, 1]], (), 1).tobytes()


def test_structs_match_the_header():
    """sizeof and offsetof as a C compiler reads include/aic_hip.h, against the ctypes mirrors and the record's dtype"""
    structs = {"aic_stale_cubes_desc": abi.StaleCubesDesc, "aic_stale_cubes_info": abi.StaleCubesInfo, "aic_stale_cube_rect": None, "aic_stale_info": abi.StaleInfo,
               "aic_stale_desc": abi.StaleDesc}
    fields = {"aic_stale_cube_rect": list(abi.STALE_CUBE_RECT_DTYPE.names), **{name: [f[0] for f in t._fields_] for name, t in structs.items() if t}}
    prints = "".join(f'printf("{name} %zu", sizeof({name}));' + "".join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields[name]) + 'printf("\\n");'
                     for name in structs)
    d = tempfile.mkdtemp(prefix="aic_stale_cubes_structs_")
    src = os.path.join(d, "s.c")
    Path(src).write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "aic_hip.h"\nint main(void) {{ {prints} return 0; }}\n')
    subprocess.run(["cc", "-I", str(ROOT / "include"), src, "-o", os.path.join(d, "s")], check=True)
    out = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out if line}
    for name, t in structs.items():
        if t:
            assert seen[name] == [C.sizeof(t)] + [getattr(t, f).offset for f in fields[name]], name
    dt = abi.STALE_CUBE_RECT_DTYPE
    assert seen["aic_stale_cube_rect"] == [dt.itemsize] + [dt.fields[f][1] for f in dt.names] == [24, 0, 4, 8, 12, 16, 20]
    assert dt == ref.CUBE_RECT_DTYPE
    assert (C.sizeof(abi.StaleCubesDesc), C.sizeof(abi.StaleCubesInfo)) == (192, 40)
    # no field of an existing struct moved
    assert seen["aic_stale_info"] == [32, 0, 8, 16, 20, 24, 28] and seen["aic_stale_desc"][0] == 48
    assert (abi.STALE_DEPTH_TEST, abi.STALE_DEPTH_BEHIND, abi.STALE_MAX_RECTS) == (1, 2, 4096) == (ref.DEPTH_TEST, ref.DEPTH_BEHIND, stale_ref.MAX_RECTS)


def test_binding():
    lib = abi.load()
    arity = {"aic_pick_stale_cubes": 6, "aic_probe_stale_cube_rects": 3, "aic_light_changed_count": 4, "aic_light_changed_take": 5}
    for name, n_args in arity.items():
        assert name in abi.ABI_SYMBOLS and hasattr(lib, name), name
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None and len(argtypes) == n_args and argtypes[0] is C.c_void_p, name
    assert lib.aic_pick_stale_cubes.argtypes[1] is lib.aic_probe_stale_cube_rects.argtypes[1] and lib.aic_pick_stale_cubes.argtypes[5]._type_ is abi.StaleCubesInfo
    for name in ("pick_stale_cubes", "probe_stale_cube_rects", "light_changed"):
        assert callable(getattr(abi.Context, name))
    assert lib.aic_abi_version() == 3
