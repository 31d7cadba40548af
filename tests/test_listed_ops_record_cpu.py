"""The calls that take a list and work on it on the device, without a GPU: tools/submit_record/listed_ops_record.cpp drives aic_trace_pixels
(csrc/aic_frame.cpp), aic_sample_luminance and aic_cursor_raycast (csrc/aic_ray_queries.cpp) and aic_pick_stale (csrc/aic_split_ops.cpp) against the recording
fake of the HIP runtime and of the kernel launchers through a fixed scenario list and prints every call with its arguments, every result and what the
context keeps. Two revisions of the host code make the same calls exactly when their records are byte-identical (tools/submit_record/build.sh says how to
compare; profiles/listed_ops_refactor.txt is such a comparison). Here: the record of the current tree, and what the comments of those files and
include/aic_hip.h promise of these calls, read from it."""
import os
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

COUNTS = (0, 1, 63, 64, 65, 2049)


@pytest.fixture(scope="module")
def record():
    """scenario name -> its lines, in the record's order"""
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_listed_ops_record_"), "listed_ops_record")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "listed_ops_record.cpp"], check=True,
                   capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    scenarios, name = {}, None
    for line in out.split("\n"):
        if line.startswith("== "):
            name = line[3:]
            assert name not in scenarios, name
            scenarios[name] = []
        elif name is not None:
            scenarios[name].append(line)
    return scenarios


def results(lines):
    """the result lines of a scenario's calls: "<entry point> rc <code>[ : <message>]" """
    return [line for line in lines if line.startswith("aic_") and " rc " in line]


def states(lines):
    return [line for line in lines if line.startswith("  state ")]


def calls(lines):
    """(result line, the runtime calls and launches recorded since the result before it) of every recorded call of a scenario"""
    out, start = [], 0
    for i, line in enumerate(lines):
        if line.startswith(("-- ", "hipFree")):
            start = i + 1
        if line.startswith("aic_") and " rc " in line:
            out.append((line, [x for x in lines[start:i] if not x.startswith("  ")]))
            start = i + 1
    return out


def test_record_is_complete(record):
    assert len(record) >= 500
    assert f"total: {len(record)} scenarios" in list(record.values())[-1]  # (the program's own count, the record's last line)
    assert not any("LEAK" in line or "FAILED" in line for lines in record.values() for line in lines)
    launchers = ("launch_trace_image", "launch_sample_luminance", "launch_cursor_raycast", "launch_pick_stale", "light_visible_bits")
    for launcher in launchers:
        assert any(line.split(" ")[0] == launcher for lines in record.values() for line in lines), launcher
    for n in COUNTS:
        for flags in (0, 8, 16, 512):  # RGBA8, AIC_FRAME_OUT_LINEAR, _COLORBUF, _SPLIT
            for layout in range(3):
                for aux in range(2):
                    assert len(results(record[f"pixels {n} {flags} {layout} {aux}"])) == 3
        # an empty list is AIC_OK and queues nothing
        for name in (f"pixels {n} 0 0 0", f"luminance {n} 0", f"cursor {n} 1", f"stale {n} 1 0"):
            made = [line for line in record[name] if line.split(" ")[0] in launchers]
            assert bool(made) == bool(n), name


def test_a_ray_query_touches_no_frame_slot(record):
    """csrc/aic_ray_queries.cpp: "all on the context's upload stream, which runs beside the frame slots: frames in flight are neither waited for nor touched"."""
    lines = record["in flight"]
    submit, queries, wait = lines.index("-- submit"), lines.index("-- queries"), lines.index("-- wait")
    stream = re.compile(r" (S\d+)\b")
    slot_streams = {s for line in lines[submit:queries] for s in stream.findall(line)}
    assert len(slot_streams) == 2  # slots 0 and 1
    asked = lines[queries:wait]
    assert [r for r in results(asked)] == ["aic_sample_luminance rc 0", "aic_cursor_raycast rc 0"]
    assert states(asked)[-1].endswith(" slot0_busy 1")
    assert any(line.startswith("launch_sample_luminance") for line in asked) and any(line.startswith("launch_cursor_raycast") for line in asked)
    used = {s for line in asked for s in stream.findall(line)}
    assert len(used) == 1 and not used & slot_streams, (used, slot_streams)
    assert not any(line.startswith("hipEvent") for line in asked)
    # ... and the frames are there to be collected afterwards
    assert results(lines[wait:]) == ["aic_render_wait rc 0"] * 2


def test_a_device_list_is_neither_staged_nor_read_back(record):
    """include/aic_hip.h, AIC_RAYS_DEVICE and AIC_PIXELS_DEVICE: "device pointers on the context's device (no staging copy, no read-back)". Read from the calls
    after a scenario's first, which made the context and the caller's own buffers ahead of it."""
    for n in COUNTS[1:]:
        for name, scratch in ((f"luminance {n} 1", " exposure_scratch 0/0 "), (f"cursor {n} 1", " cursor_scratch 0/0 ")):
            lines = record[name]
            assert all(scratch in state for state in states(lines)), name
            later = [(result, made) for result, made in calls(lines)[1:] if not result.startswith("aic_update_cubes")]
            assert later and all(result.endswith(" rc 0") for result, _ in later), name
            for _, made in later:
                assert any(line.startswith("launch_") for line in made), name
                assert not any(line.startswith("hipMalloc") for line in made), (name, made)
                # (after a scene write the bitmap of visible blocks is staged again, 2048 words: the scene's, not the list's)
                assert all(" bytes 8192 kind 1 " in line for line in made if line.startswith("hipMemcpy")), (name, made)
        for flags in (0, 8, 16, 512):
            for layout in (1, 2):
                for aux in range(2):
                    name = f"pixels {n} {flags} {layout} {aux}"
                    traced = calls(record[name])
                    assert len(traced) == 3 and all(result == "aic_trace_pixels rc 0" for result, _ in traced), name
                    assert all(" out 0/0 staging 0/0 " in state for state in states(record[name])), name
                    for _, made in traced[1:]:
                        assert any(line.startswith("launch_trace_image") for line in made), name
                        assert not any(line.startswith(("hipMalloc", "hipMemcpy")) for line in made), (name, made)
    # a host list of the same shape is staged, its results copied back and its hit records read back
    for _, made in calls(record["pixels 65 512 0 1"])[1:]:
        assert any(line.startswith("hipMemcpyAsync") and " bytes 260 kind 1 " in line for line in made)          # 65 pixels in
        assert any(line.startswith("hipMemcpyAsync host <-") and " bytes 780 kind 2 " in line for line in made)  # 65 x 12 bytes out
        assert any(line.startswith("hipMemcpy host <-") for line in made)                                       # the hit records


def test_the_visible_bitmap_is_made_once_per_scene_version(record):
    """csrc/aic_ctx.h, Layer::visible_bits: "made by the first sample after `version` moved"."""
    for n in COUNTS[1:]:
        for on_device in range(2):
            lines = record[f"luminance {n} {on_device}"]
            traced = calls(lines)
            assert [result for result, _ in traced] == ["aic_sample_luminance rc 0"] * 2 + ["aic_update_cubes rc 0", "aic_sample_luminance rc 0"]
            made = [sum(line.startswith("light_visible_bits") for line in call) for _, call in traced]
            staged = [sum(" bytes 8192 kind 1 " in line for line in call) for _, call in traced]
            assert made == [1, 0, 0, 1] and staged == made, (n, on_device, made, staged)
            versions = [re.search(r" version (\d+) visible_version (-?\d+) ", line).groups() for line in states(lines)]
            assert len(versions) == 3 and all(v == seen for v, seen in versions) and versions[0] == versions[1] != versions[2]
    # an empty list makes no bitmap
    assert not any(line.startswith("light_visible_bits") for line in record["luminance 0 0"])


def test_a_refused_call_leaves_the_state_and_queues_nothing(record):
    rejections = {name: lines for name, lines in record.items() if name.startswith("reject: ")}
    assert len(rejections) >= 65
    last_state = None
    for name, lines in record.items():  # (in the record's order: the rejections share one context)
        if name in rejections:
            got = results(lines)
            # AIC_ERR_INVALID or AIC_ERR_UNSUPPORTED and its message under the entry point's name (without a context there is nowhere to keep one)
            assert len(got) == 1 and re.search(r" rc [15] : aic_\w+: | rc 1 : no context$", got[0]), (name, got)
            assert not any(line.startswith(("hip", "launch_", "light_")) for line in lines), (name, lines)
            if " rc 1 : aic_" in got[0] and "no context" not in name:
                assert states(lines) == [last_state], name
        if states(lines):
            last_state = states(lines)[-1]
    busy = "a submitted frame still occupies slot 0 (aic_render_wait it first)"
    for what, who in {"pixels": "aic_trace_pixels", "pixels, a device list": "aic_trace_pixels", "stale": "aic_pick_stale", "stale, n = 0": "aic_pick_stale"}.items():
        assert results(rejections[f"reject: busy: {what}"])[0].endswith(f" rc 1 : {who}: {busy}")
        assert states(rejections[f"reject: busy: {what}"])[0].endswith(" slot0_busy 1")
    assert [r.split(" rc ")[1] for r in results(record["rejections: the frame is waited for and every call runs"])] == ["0"] * 5


def test_a_failed_runtime_call_leaves_the_context_usable(record):
    failed = {name: lines for name, lines in record.items() if name.startswith("failures: ") and not name.endswith(", the good call")}
    assert len(failed) >= 80
    for entry in ("pixels 0", "pixels 1", "luminance 0", "luminance 1", "cursor 0", "cursor 1", "stale looked at", "stale not looked at"):
        assert results(record[f"failures: {entry}, the good call"])[-1].endswith(" rc 0")
        assert sum("-- the same call again" in lines for name, lines in failed.items() if name.startswith(f"failures: {entry} ")) >= 3, entry
    for name, lines in failed.items():
        if "-- the same call again" not in lines:  # (the scenario that ends a function's turn: the call does not reach an nth such call)
            assert all(result.endswith(" rc 0") for result in results(lines)), name
            continue
        assert sum(line.endswith(" FAILS") for line in lines) == 1, name
        again = lines.index("-- the same call again")
        first, second = results(lines[:again]), results(lines[again:])
        assert len(first) == 1 and len(second) == 1, name
        if " hipMemsetAsync " not in name:  # (clearing the counters behind a frame: the next frame clears them itself)
            assert not first[0].endswith(" rc 0"), (name, first)
        # (a listed trace that fails behind its submit leaves the frame uncollected: it occupies slot 0 until aic_render_wait, and the next one is refused)
        busy = " rc 1 : aic_trace_pixels: a submitted frame still occupies slot 0 (aic_render_wait it first)"
        assert second[0].endswith(" rc 0") or (name.startswith("failures: pixels") and second[0].endswith(busy)), (name, second)
