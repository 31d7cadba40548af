"""The operations on a resident Split frame without a GPU: tools/submit_record/split_ops_record.cpp drives csrc/aic_split_ops.cpp (aic_reproject_split,
aic_pick_pixels, aic_present_split, aic_present_split_lines) against the recording fake of the HIP runtime and of the kernel launchers through a fixed
scenario list and prints every call with its arguments, every result and what the context keeps. Two revisions of the host code make the same calls
exactly when their records are byte-identical (tools/submit_record/build.sh says how to compare; profiles/split_ops_refactor.txt is such a comparison).
Here: the record of the current tree, and what include/aic_hip.h promises of these calls, read from it."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

QUEUED = ("hipMalloc", "hipEventRecord", "hipMemcpyAsync", "hipMemsetAsync", "launch_")


@pytest.fixture(scope="module")
def record():
    """scenario name -> its lines"""
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_split_ops_record_"), "split_ops_record")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "split_ops_record.cpp"], check=True,
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


def test_record_is_complete(record):
    assert len(record) >= 800
    assert f"total: {len(record)} scenarios" in list(record.values())[-1]  # (the program's own count, the record's last line)
    assert not any("LEAK" in line or "FAILED" in line for lines in record.values() for line in lines)
    # every launcher is reached, with its arguments on the lines below its name
    for launcher in ("launch_reproject", "launch_pick", "launch_present", "launch_present_scene", "launch_present_lines"):
        assert any(line.split(" ")[0] == launcher for lines in record.values() for line in lines), launcher


def test_a_rejection_queues_and_allocates_nothing(record):
    rejections = {name: lines for name, lines in record.items() if name.startswith("reject: ")}
    assert len(rejections) >= 90
    for name, lines in rejections.items():
        got = results(lines)
        assert len(got) == 1 and " rc 1 : " in got[0], (name, got)  # AIC_ERR_INVALID and its message
        assert not any(line.startswith(QUEUED) for line in lines[: lines.index(got[0])]), (name, lines)
    # while a frame occupies slot 0 every entry point refuses under its own name; without lines aic_present_split_lines is aic_present_split
    who = {"reproject": "aic_reproject_split", "pick": "aic_pick_pixels", "present": "aic_present_split", "present with lines": "aic_present_split_lines",
           "present through aic_present_split_lines, no lines": "aic_present_split"}
    for what, name in who.items():
        assert results(rejections[f"reject: busy: {what}"])[0].endswith(f" rc 1 : {name}: a submitted frame still occupies slot 0 (aic_render_wait it first)")


def test_no_lines_is_aic_present_split(record):
    """include/aic_hip.h: "lines == NULL or n_lines == 0: the call is aic_present_split itself -- the same launches, no extra scratch, lines_info zeroed"."""
    def comparable(lines):
        lines = [line for line in lines if not line.startswith("  lines_info ")]
        return [line.replace("aic_present_split_lines rc", "aic_present_split rc") if line.startswith("aic_present_split_lines rc") else line for line in lines]

    plain = {name: lines for name, lines in record.items() if name.startswith("present ") and name.endswith(" 0")}
    assert len(plain) == 64
    for name, lines in plain.items():
        assert len(results(lines)) == 2 and all(r == "aic_present_split rc 0" for r in results(lines)), name
        for form in (1, 2):  # a list of no lines; no list
            other = record[name[:-1] + str(form)]
            assert [line for line in other if line.startswith("  lines_info ")] == ["  lines_info clipped_away 0 fragments 0 passed 0 pixels 0"] * 2
            assert comparable(other) == lines, (name, form)
    assert any(line.startswith("launch_present") for lines in plain.values() for line in lines)
    assert not any(line.startswith(("launch_present_scene", "launch_present_lines")) for lines in plain.values() for line in lines)


def test_a_failed_runtime_call_leaves_the_context_usable(record):
    failed = {name: lines for name, lines in record.items() if name.startswith("failures: ") and not name.endswith(", the good call")}
    assert len(failed) >= 70
    for entry in ("reproject", "pick", "present 0", "present 1", "lines 0 0", "lines 0 1", "lines 1 0", "lines 1 1"):
        assert results(record[f"failures: {entry}, the good call"])[-1].endswith(" rc 0")
        assert any(name.startswith(f"failures: {entry} ") for name in failed), entry
    for name, lines in failed.items():
        assert sum(line.endswith(" FAILS") for line in lines) == 1, name
        again = lines.index("-- the same call again")
        first, second = results(lines[:again]), results(lines[again:])
        assert first and not first[-1].endswith(" rc 0"), (name, first)
        assert len(second) == 1 and second[0].endswith(" rc 0"), (name, second)
