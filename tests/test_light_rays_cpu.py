"""aic_light_rays without a GPU: the host's maker of the lines (aic_light_rays_wireframe) against the restatement's
(tests/light_rays_ref.py) byte for byte, aic_light_rays_bound against the chart and against every count the restatement produces, and the call's host
side -- aic_light_rays in aic_light_rays_host.cpp -- driven by tools/submit_record/light_rays_record.cpp against the recording fake of the HIP runtime.
That program has its own main and is built here with -fsanitize=address,undefined: host code only, nothing of it is loaded into Python."""
import ctypes
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import oracle
from all_is_cubes_amd import abi
from tests import light_rays_ref as ref

ROOT = Path(__file__).resolve().parent.parent
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
CASES = ["closed_cell", "spread_6", "spread_30", "slab_6", "slab_30", "edges"]


def test_the_library_exports_the_calls():
    lib = abi.load()
    for name in ("aic_light_rays", "aic_light_rays_bound", "aic_light_rays_wireframe"):
        assert hasattr(lib, name)
    assert abi.LIGHT_CUBE_INFO_DTYPE.itemsize == 32 and abi.LIGHT_RAY_DTYPE.itemsize == 40 and abi.LINE_VERTEX_DTYPE.itemsize == 28


# ---- the lines ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_wireframe_equals_the_restatement(case):
    infos, rays, lines, totals = ref.answer(case)
    assert totals == (len(rays), 12 * len(infos) + 29 * len(rays)) and len(lines) == 2 * totals[1]
    at = 0
    for info in infos:
        own = rays[info["first_ray"]:info["first_ray"] + info["n_rays"]]
        got = abi.light_rays_wireframe(info, own)
        assert len(got) == 2 * (12 + 29 * len(own))
        assert got.tobytes() == lines[at:at + len(got)].tobytes(), tuple(info["cube"])
        at += len(got)
    assert at == len(lines)


def hand_records():
    """Records built by hand around the cube (4, -7, 2): the six face directions (a ray along +Y or -Y is parallel to `up`: the perp1 fallback of
    ray.rs:136-139), a short diagonal, and far ones whose arrowhead takes the 0.125 cap."""
    cube = (4, -7, 2)
    recs = []
    for f, n in enumerate(ref.NORMALS):
        trigger = tuple(c + v for c, v in zip(cube, n))
        recs.append((trigger, cube, (10 * f, 200, 255, 255), np.array([0.25 * f, 1.5, 1e-3], np.float32)))
    for trigger, value_cube in (((5, -6, 2), (5, -7, 2)), ((4, 12, 2), (4, 11, 2)), ((4, -30, 2), (4, -29, 2)), ((-20, 5, 31), (-19, 5, 31)), ((4, -7, 30), (4, -7, 29)),
                                ((2147483647, -2147483648, 0), (2147483646, -2147483648, 0))):
        recs.append((trigger, value_cube, (0, 0, 0, 1), np.array([3.0, 0.0, 65504.0], np.float32)))
    return cube, ref.records_array(recs)


def test_wireframe_of_records_built_by_hand():
    cube, rays = hand_records()
    info = np.zeros(1, abi.LIGHT_CUBE_INFO_DTYPE)
    info["cube"], info["n_rays"] = cube, len(rays)
    got = abi.light_rays_wireframe(info, rays)
    want = ref.wireframe(cube, rays)
    assert got.tobytes() == want.tobytes()
    # the layout: the cube's box, then per record the value cube's box and the arrow; colours as the reference gives them
    assert np.array_equal(got["color"][:24], np.tile(np.array([0.8, 0.8, 1.0, 1.0], np.float32), (24, 1)))
    assert np.array_equal(got["position"][0], np.array([3.9, -7.1, 1.9], np.float32)) and np.array_equal(got["position"][23], np.array([5.1, -5.9, 3.1], np.float32))
    first_arrow = got[2 * (12 + 12):2 * (12 + 29)]
    assert np.array_equal(first_arrow["color"][:, :3], np.tile(rays[0]["light_from_struck_face"], (34, 1))) and (first_arrow["color"][:, 3] == 1.0).all()
    assert np.array_equal(first_arrow["position"][0], np.array([4.5, -6.5, 2.5], np.float32)) and np.array_equal(first_arrow["position"][1], np.array([4.0, -6.5, 2.5], np.float32))
    # +Y and -Y (records 4 and 1) took the fallback: their cones are circles in the plane y = const
    for r in (1, 4):
        arrow = got[2 * (12 + 29 * r + 12):2 * (12 + 29 * (r + 1))]
        ring = arrow["position"][2::4]
        assert len(ring) == 8 and (ring[:, 1] == ring[0, 1]).all() and len({tuple(p) for p in ring}) == 8


def test_wireframe_rejects_null_pointers():
    lib = abi.load()
    lib.aic_light_rays_wireframe.restype = ctypes.c_int
    lib.aic_light_rays_wireframe.argtypes = [ctypes.c_void_p] * 4
    info = np.zeros(1, abi.LIGHT_CUBE_INFO_DTYPE)
    out = np.zeros(24, abi.LINE_VERTEX_DTYPE)
    n = ctypes.c_uint32(0)
    assert lib.aic_light_rays_wireframe(None, None, out.ctypes.data, ctypes.addressof(n)) == 1
    assert lib.aic_light_rays_wireframe(info.ctypes.data, None, None, ctypes.addressof(n)) == 1
    assert lib.aic_light_rays_wireframe(info.ctypes.data, None, out.ctypes.data, None) == 1
    info["n_rays"] = 1
    assert lib.aic_light_rays_wireframe(info.ctypes.data, None, out.ctypes.data, ctypes.addressof(n)) == 1
    info["n_rays"] = 0
    assert lib.aic_light_rays_wireframe(info.ctypes.data, None, out.ctypes.data, ctypes.addressof(n)) == 0 and n.value == 12


# ---- the bound ---------------------------------------------------------------------------------------------------------

def chart_bound(maximum_distance: int) -> int:
    """Bundles within the distance, the root apart, with no child within it, counted in the oracle's chart: a record ends its bundle, so a cube's records
    are pairwise off each other's root paths, and these are the most bundles that can be."""
    _, children = ref.chart()
    max2 = maximum_distance * maximum_distance
    count = 0
    stack = [(0, 0, 0, 0)]
    while stack:
        node, x, y, z = stack.pop()
        within_children = 0
        for f, child in enumerate(children[node]):
            if child:
                n = ref.NORMALS[f]
                c = (x + n[0], y + n[1], z + n[2])
                if c[0] * c[0] + c[1] * c[1] + c[2] * c[2] <= max2:
                    within_children += 1
                    stack.append((child, *c))
        if node != 0 and within_children == 0:
            count += 1
    return count


@pytest.mark.parametrize("maximum_distance", [0, 1, 2, 6, 30, 255])
def test_bound_is_counted_in_the_chart(maximum_distance):
    assert abi.light_rays_bound(maximum_distance) == chart_bound(maximum_distance)


def test_bound_values_and_range():
    assert abi.light_rays_bound(0) == 0 and abi.light_rays_bound(1) == 6
    assert abi.light_rays_bound(30) == abi.light_rays_bound(255) == 602  # the chart's rays
    assert abi.light_rays_bound(-1) == 0 and abi.light_rays_bound(256) == 0
    assert all(abi.light_rays_bound(d) <= abi.light_rays_bound(d + 1) for d in range(0, 40))


@pytest.mark.parametrize("case", CASES)
def test_bound_holds_for_every_count_the_restatement_produces(case):
    infos = ref.answer(case)[0]
    assert int(infos["n_rays"].max()) <= abi.light_rays_bound(ref.cases()[case][2])


def test_closed_cell_by_hand():
    """The six records of the closed cell: trigger = the face neighbour, value = the centre, colour = emission + face colour x the centre's light."""
    infos, rays, _, _ = ref.answer("closed_cell")
    sp, t = ref.scene("closed_cell")
    centre = np.asarray(sp.light).reshape(3, 3, 3, 4)[1, 1, 1]
    value = t.lut[centre[:3]]
    assert infos["n_rays"][0] == 6 and len(rays) == 6
    for f, r in enumerate(rays):
        assert tuple(r["trigger_cube"]) == tuple(1 + v for v in ref.NORMALS[f]) and tuple(r["value_cube"]) == (1, 1, 1) and np.array_equal(r["value"], centre)
        colour, emission = (ref.LAMP_COLOR, ref.LAMP_EMISSION) if f == 0 else ((0.5, 0.25, 0.75, 1.0), (0.0, 0.0, 0.0))
        want = np.array(emission, np.float32) + np.array(colour[:3], np.float32) * value
        assert np.array_equal(r["light_from_struck_face"], want.astype(np.float32))


# ---- the call's host side, against the recording fake ----------------------------------------------------------------------

QUEUED = ("hipMalloc", "hipMemcpyAsync", "hipMemcpy ", "hipMemsetAsync", "launch_", "light_rays_derived")
REJECTIONS = ["no context", "no cubes", "unknown flag", "unknown flag beside AIC_LIGHT_RAYS_DEVICE", "a layer with no space", "no such layer", "negative maximum_distance",
              "maximum_distance 256", "too many cubes", "device rays off by 2", "device lines off by 1"]


@pytest.fixture(scope="module")
def record():
    """scenario name -> its lines, from the sanitizer build; the run itself must be clean"""
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_light_rays_record_"), "light_rays_record")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "light_rays_record.cpp", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"], check=True, capture_output=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    scenarios, name = {}, None
    for line in run.stdout.split("\n"):
        if line.startswith("== "):
            name = line[3:]
            scenarios[name] = []
        elif name is not None:
            scenarios[name].append(line)
    return scenarios


def split_at(lines, marker):
    """the stretches of `lines` that follow each line beginning with `marker`, keyed by the rest of that line"""
    out, key = {}, None
    for line in lines:
        if line.startswith(marker):
            key = line[len(marker):]
            out[key] = []
        elif line.startswith("-- "):
            key = None
        elif key is not None:
            out[key].append(line)
    return out


@needs_hipcc
def test_record_has_no_failed_expectation(record):
    assert "end" in record
    bad = [(name, line) for name, lines in record.items() for line in lines if line.startswith("FAILED") or line.startswith("LEAK")]
    assert bad == []


@needs_hipcc
def test_every_rejection_leaves_no_launch(record):
    rejected = split_at(record["rejections"], "-- reject: ")
    assert list(rejected) == REJECTIONS
    for what, lines in rejected.items():
        assert len(lines) == 1 and lines[0].startswith("aic_light_rays rc 1 : ") and (what == "no context" or "aic_light_rays: " in lines[0]), (what, lines)
        assert not any(q in line for line in lines for q in QUEUED)
    # ... and the context is usable: the call after each one runs the walk, the scan and the emitters
    after = split_at(record["rejections"], "-- after: ")
    for what, lines in after.items():
        assert [line.split(" ")[0] for line in lines if line.startswith("launch_")] == ["launch_light_rays_walk", "launch_light_rays_scan", "launch_light_rays_emit"], what
        assert lines[-1] == "aic_light_rays rc 0"


@needs_hipcc
def test_a_pending_light_update_is_finished_first(record):
    lines = record["a pending light update is finished first"]
    first = lines.index("light_job_finish: a pending update")
    # nothing of the call is queued before the update is finished: the tables, the staging and the launches all follow it
    own = [i for i, line in enumerate(lines) if line.startswith(("light_rays_", "launch_light_rays_"))]
    assert own and first < min(own)
    assert lines.count("light_job_finish: a pending update") == 1
    rejected = split_at(lines, "-- a rejected call")
    assert list(rejected.values())[0][0] == "aic_light_rays rc 1 : aic_light_rays: maximum_distance is a u8"


def call_lines(lines, turn):
    return split_at(lines, "-- call ")[str(turn)]


@needs_hipcc
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_host_lists_are_staged_and_device_lists_stage_nothing(record, n):
    host, device = call_lines(record[f"launch {n} 0 {2 * n}"], 0), call_lines(record[f"launch {n} 1 {2 * n}"], 0)

    def scratch(lines):  # the bytes of the call's scratch: the third allocation, after the tree's and the derived properties'
        return [int(line.split(" ")[1]) for line in lines if line.startswith("hipMalloc ")][2]

    def emit(lines):
        return next(line for line in lines if line.startswith("launch_light_rays_emit"))

    ray_bytes, line_bytes = 40 * 2 * n, 28 * 2 * (12 * n + 29 * 2 * n)
    assert scratch(host) - scratch(device) >= ray_bytes + line_bytes  # (DevBuf::ensure over-allocates by a quarter)
    # the host call's emitters write into the context's scratch and two copies bring the lists back; the device call's write into the caller's buffers
    scratch_ordinal = f"A{[line for line in host if line.startswith('hipMalloc ')][2].split('-> A')[1]}+"
    assert emit(host).count(scratch_ordinal) == 2
    back = [line for line in host if line.startswith("hipMemcpyAsync host <- ")]
    assert [int(line.split(" bytes ")[1].split(" ")[0]) for line in back][-2:] == [ray_bytes, line_bytes]
    assert emit(device).count("+0 ") == 2 and not [line for line in device if line.startswith("hipMemcpyAsync host <- ") and int(line.split(" bytes ")[1].split(" ")[0]) > 32 * n]
    # everything runs on the upload stream: one stream in the whole call
    streams = {tok for line in host + device for tok in line.split(" ") if tok.startswith("S") and tok[1:].isdigit()}
    assert len(streams) == 1
    # the second call allocates nothing and copies no table
    again = call_lines(record[f"launch {n} 0 {2 * n}"], 1)
    assert not any(line.startswith("hipMalloc") or line.startswith("light_rays_") for line in again)


@needs_hipcc
def test_tables_follow_the_distance_and_the_scene(record):
    lines = record["tables: another distance makes the tree again, a scene write the derived properties"]
    assert [line for line in lines if line.startswith("light_rays_tree")] == ["light_rays_tree 6", "light_rays_tree 7"]
    assert len([line for line in lines if line.startswith("light_rays_derived")]) == 2


@needs_hipcc
def test_a_failed_runtime_call_is_reported_and_the_next_call_works(record):
    failures = {name: lines for name, lines in record.items() if name.startswith("failures: ")}
    assert len(failures) == 31
    for name, lines in failures.items():
        again = lines.index("-- the same call again")
        assert any(line.endswith(" FAILS") for line in lines[:again]), name
        rcs = [line for line in lines if line.startswith("aic_light_rays rc ")]
        assert len(rcs) == 2 and not rcs[0].startswith("aic_light_rays rc 0") and rcs[1] == "aic_light_rays rc 0", name


@needs_hipcc
def test_cursor_lines_are_one_device_list(record):
    lines = record["cursor lines: one device list"]
    calls = split_at(lines, "-- call ")
    for turn in ("0", "1"):
        assert "aic_light_rays_cursor_lines rc 0" in calls[turn]
        # the caller's lines go to the head of the list, the cube's are written behind them by the emitters: nothing of them is copied
        (emit,) = [line for line in calls[turn] if line.startswith("launch_light_rays_emit")]
        (listed,) = [line for line in calls[turn] if line.startswith("  list ")]
        base = listed.split(" ")[3]
        assert base.endswith("+0") and f" lines {base[:-1]}{28 * 2 * 28} " in emit and listed.endswith(" n_lines 98")
        staged = [line for line in calls[turn] if line.startswith(f"hipMemcpyAsync {base} <- host bytes {28 * 2 * 28} ")]
        assert len(staged) == 1
        assert not [line for line in calls[turn] if line.startswith("hipMemcpyAsync host <- ") and int(line.split(" bytes ")[1].split(" ")[0]) > 32]
    assert not any(line.startswith("hipMalloc") for line in calls["1"])
    rejected = split_at(lines, "-- reject: ")
    assert len(rejected) == 7
    for what, got in rejected.items():
        assert got[0].startswith("aic_light_rays_cursor_lines rc 1 : aic_light_rays_cursor_lines: "), (what, got)  # (the context's teardown follows the last)
        assert not any(line.startswith(("hipMalloc", "hipMemcpyAsync", "launch_", "light_rays_")) for line in got), what
