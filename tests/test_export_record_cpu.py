"""aic_export_split's host side without a GPU: tools/submit_record/split_ops_record.cpp drives csrc/aic_split_ops.cpp against the recording fake of the HIP
runtime and of the kernel launchers, and its export scenarios are read here -- what is launched for each combination of planes and targets, what a
rejection leaves alone, what a failed runtime call leaves usable (tests/test_split_ops_record_cpu.py applies its rules to every scenario by name; the
ones below are the export's own). The program has its own main and is built here with -fsanitize=address,undefined: host code only, nothing of it is
loaded into Python."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

QUEUED = ("hipMalloc", "hipEventRecord", "hipMemcpyAsync", "hipMemsetAsync", "launch_")
REJECTIONS = ["no context", "no desc", "no src", "nothing asked for", "nothing asked for of the host", "src off by 4", "color_out off by 2", "depth_out off by 1",
              "color_out is src", "depth_out inside src", "depth_out is color_out", "color_out inside depth_out", "src too wide", "src too high", "out too wide",
              "out too high", "more than 2^31 pixels", "src of no width", "src of no height", "NaN in ipzw", "infinity in ipzw", "unknown flag"]


@pytest.fixture(scope="module")
def record():
    """scenario name -> its lines, from the sanitizer build; the run itself must be clean"""
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_export_record_"), "split_ops_record")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "split_ops_record.cpp", "-Xarch_host",
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


def results(lines):
    return [line for line in lines if line.startswith("aic_export_split rc ")]


def launches(lines):
    return [line for line in lines if line.startswith("launch_export ")]


def test_no_scenario_of_the_export_leaks_or_fails_to_fail(record):
    ours = {name: lines for name, lines in record.items() if "export" in name}
    assert len(ours) >= 100
    assert not any("LEAK" in line or "FAILED" in line for lines in ours.values() for line in lines)
    assert not any(name.startswith("present ") for name in ours)


def test_planes_and_targets(record):
    """export <src w> <src h> <out w> <out h> <planes: bit 0 colour, bit 1 depth> <to_device>: two calls with info, then (with a plane) one without."""
    for size, npix in (("20 12 40 24", 40 * 24), ("33 17 16 8", 16 * 8), ("33 17 33 17", 33 * 17), ("1 1 5 3", 15)):
        for planes in range(4):
            for to_device in range(2):
                lines = record[f"export {size} {planes} {to_device}"]
                n_calls = 3 if planes else 2
                assert results(lines) == ["aic_export_split rc 0"] * n_calls, (size, planes, to_device)
                got = launches(lines)
                assert len(got) == n_calls and len(set(got)) == 1  # (the later calls find the counters and the staging where the first left them)
                launch = got[0]
                assert (" color null" in launch) == (not planes & 1) and (" depth null" in launch) == (not planes & 2), launch
                if planes == 3 and not to_device:  # the two planes share the staging: colour first, depth npix * 4 bytes behind it
                    color, depth = launch.split(" color ")[1].split(" ")[0], launch.split(" depth ")[1].split(" ")[0]
                    assert color.split("+")[0] == depth.split("+")[0] and int(depth.split("+")[1]) - int(color.split("+")[1]) == npix * 4
                # what is copied back: the 64 slots of counters (128 bytes each) always, and each plane asked of the host
                back = [line for line in lines if line.startswith("hipMemcpyAsync host <- ")]
                per_call = 1 + (0 if to_device else bin(planes).count("1"))
                assert len(back) == per_call * n_calls
                assert sum(" bytes 8192 " in line for line in back) == n_calls
                assert sum(f" bytes {npix * 4} " in line for line in back) == (per_call - 1) * n_calls
                # allocated by the first call alone: the counters, and the staging of a host target
                first_call = lines.index("aic_export_split rc 0")
                assert not any(line.startswith("hipMalloc") for line in lines[first_call:]), "a later call allocated again"
                # the info of a call that wants it: the fake's time, and statistics of a frame of zeros -- no surface
                infos = [line for line in lines if line.startswith("  info kernel_ms ")]
                assert infos[0] == infos[1] == "  info kernel_ms 0x1p+0 n_surface 0 depth_min 0x0p+0 depth_max 0x0p+0 reserved 0 0 0 0"


def test_an_empty_output_queues_nothing(record):
    for size in ("0 0 0 0", "8 8 0 8"):
        for planes in range(4):
            for to_device in range(2):
                lines = record[f"export {size} {planes} {to_device}"]
                assert results(lines) and all(r == "aic_export_split rc 0" for r in results(lines))
                assert not launches(lines)
                first = lines.index(results(lines)[0])
                last = len(lines) - 1 - lines[::-1].index(results(lines)[-1])
                setup_done = max(i for i, line in enumerate(lines[:first]) if line.startswith("hipMalloc"))  # (the caller's own buffers)
                assert not any(line.startswith(QUEUED) for line in lines[setup_done + 1:last]), (size, planes, to_device)
                assert "  export state counts 0/0" in lines and not any(line.startswith("  export state counts") and line != "  export state counts 0/0" for line in lines)
                assert all(line.endswith("n_surface 0 depth_min 0x0p+0 depth_max 0x0p+0 reserved 0 0 0 0") for line in lines if line.startswith("  info kernel_ms 0x0p+0"))
                assert sum(line.startswith("  info kernel_ms 0x0p+0") for line in lines) == 2


def test_every_rejection_is_recorded_under_the_entry_points_name(record):
    for what in REJECTIONS + ["busy: export"]:
        name = f"reject: {what}" if what.startswith("busy") else f"reject: export: {what}"
        lines = record[name]
        got = [line for line in lines if line.startswith("aic_") and " rc " in line]
        assert len(got) == 1 and got[0].startswith("aic_export_split rc 1 : "), (name, got)
        if what != "no context":  # (no context: no message to keep)
            assert got[0].startswith("aic_export_split rc 1 : aic_export_split: "), (name, got)
        assert not any(line.startswith(QUEUED) for line in lines[: lines.index(got[0])]), name
        assert "  export state counts 0/0" in lines or what == "no context", name  # nothing allocated either
    assert record["reject: busy: export"][0].endswith("aic_export_split: a submitted frame still occupies slot 0 (aic_render_wait it first)")
    assert results(record["export: after a frame was waited for"]) == ["aic_export_split rc 0"]


def test_a_failed_runtime_call_leaves_the_context_usable(record):
    for to_device in range(2):
        assert results(record[f"failures: export {to_device}, the good call"]) == ["aic_export_split rc 0"]
        failed = {name: lines for name, lines in record.items() if name.startswith(f"failures: export {to_device} ")}
        kinds = {name.split(" ")[3] for name in failed}
        assert {"hipSetDevice", "hipMalloc", "hipMemcpyAsync", "hipEventRecord", "hipStreamSynchronize", "hipEventElapsedTime", "launch_export"} <= kinds, kinds
        assert sum(name.split(" ")[3] == "hipMalloc" for name in failed) == (1 if to_device else 2)  # the counters; the staging
        assert sum(name.split(" ")[3] == "hipMemcpyAsync" for name in failed) == (1 if to_device else 3)
        for name, lines in failed.items():
            assert sum(line.endswith(" FAILS") for line in lines) == 1, name
            again = lines.index("-- the same call again")
            first, second = results(lines[:again]), results(lines[again:])
            assert len(first) == 1 and first[0].startswith("aic_export_split rc ") and not first[0].endswith(" rc 0"), (name, first)
            assert second == ["aic_export_split rc 0"], (name, second)


def test_the_size_policy_is_recorded(record):
    lines = record["export: size policy"]
    assert "aic_export_size 640x480 cap 0x1.2cp+18 rc 0 -> 640x480" in lines
    assert "aic_export_size 1920x1080 cap 0x1.2cp+18 rc 0 -> 740x416" in lines
    assert "aic_export_size 0x7 cap 0x1p+0 rc 0 -> 0x7" in lines
    assert "aic_export_size invalid rc 1 1 1 1" in lines
