"""The frame path without a GPU: tools/submit_record builds the host side of the C ABI (csrc/aic_abi.cpp, csrc/aic_frame.cpp) against a recording fake of the
HIP runtime and of the kernel launchers, drives it through a fixed scenario list and prints every call. Two revisions of the host code make the same calls
exactly when their records are byte-identical (tools/submit_record/build.sh says how to compare; profiles/frame_submit_refactor.txt is such a comparison).
Here: the record of the current tree, and three behaviours the comments of aic_frame.cpp and aic_ctx.h promise, read from it."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def record():
    """scenario name -> its lines"""
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_submit_record_"), "submit_record")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe], check=True, capture_output=True)
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


def frames_of(lines):
    """The three frames of a "sequence" scenario: per frame, the calls ahead of its first trace launch, that launch's sub-frame 0, and the calls behind it."""
    frames = []
    for line in lines:
        if line.startswith("-- frame "):
            frames.append({"ahead": [], "sub0": None, "behind": []})
        elif frames:
            f = frames[-1]
            if f["sub0"] is None and line.startswith("  sub 0 "):
                words = line.split()
                f["sub0"] = {k: words[words.index(k) + 1] for k in ("tile_order", "tile_cost", "queue_start")}
            elif not line.startswith("  "):
                f["behind" if f["sub0"] else "ahead"].append(line)
    assert len(frames) == 3 and all(f["sub0"] for f in frames)
    for f in frames:
        assert f["ahead"][-1].startswith("launch_trace_image") and f["ahead"][-2].startswith("hipEventRecord"), f["ahead"]
    return frames


def static_order(frame):
    """the order buffer of the frame's launch_order_tiles with no cost record (the per-shape index order), or None"""
    made = [line.split() for line in frame["ahead"] if line.startswith("launch_order_tiles cost null ")]
    assert len(made) <= 1
    return made[0][made[0].index("order") + 1] if made else None


def test_record_is_complete(record):
    assert len(record) >= 400
    assert f"total: {len(record)} scenarios" in list(record.values())[-1]  # (the driver's own count, the record's last line)
    assert not any("LEAK" in line or "FAILED" in line for lines in record.values() for line in lines)
    for name in ("same camera", "moved camera", "changed shape and back"):
        for mode in range(3):
            assert f"sequence {name} {mode}" in record


def test_second_identical_frame_starts_with_its_trace(record):
    """aic_ctx.h SubSlot: "A frame alone then starts with its trace launch": what a frame needs cleared or ordered was queued behind the slot's previous frame."""
    for mode in (0, 1):  # aic_render, aic_render_submit (over a UI space: the pre-pass clears its own dispenser, behind the first launch)
        frames = frames_of(record[f"sequence same camera {mode}"])
        assert any(line.startswith("hipMemsetAsync") for line in frames[0]["ahead"])
        assert static_order(frames[0]) is not None
        for f in frames[1:]:
            ahead = [line for line in f["ahead"] if not line.startswith(("hipMalloc", "hipFree"))]  # (mode 0: the driver's own output buffer)
            assert len(ahead) == 2 and ahead[0].startswith("hipEventRecord") and ahead[1].startswith("launch_trace_image"), ahead
            assert not any(line.startswith(("hipMemsetAsync", "launch_order_tiles")) for line in f["ahead"])


def test_moved_camera_takes_the_static_order(record):
    """aic_frame.cpp record_predicts: "A stale order is worse than none"."""
    lines = record["sequence moved camera 0"]
    frames = frames_of(lines)
    static = static_order(frames[0])
    job = next(line.split() for line in lines if line.startswith("  job 0 "))
    recorded = job[job.index("order") + 1]
    assert static and recorded and static != recorded
    # frame 0: nothing recorded yet; frame 1: the camera moved five cubes; frame 2: it did not move again, so the order frame 1 recorded predicts it
    assert [f["sub0"]["tile_order"] for f in frames] == [static, static, recorded]
    assert static_order(frames[1]) is None and static_order(frames[2]) is None  # (made once per frame shape)
    same = frames_of(record["sequence same camera 0"])
    assert [f["sub0"]["tile_order"] for f in same] == [static, recorded, recorded]


def test_changed_shape_restages_the_pixel_edges(record):
    """aic_ctx.h FrameSlot::edges: the table belongs to the slot's frame shape (width + 1, then height + 1 doubles), staged before the call returns."""
    def staged(frame):
        copies = [i for i, line in enumerate(frame["ahead"]) if line.startswith("hipMemcpyAsync") and " kind 1 " in line]
        for i in copies:
            assert frame["ahead"][i + 1].startswith("hipStreamSynchronize")
        return [int(frame["ahead"][i].split()[frame["ahead"][i].split().index("bytes") + 1]) for i in copies]

    widths = (640, 320, 640)
    frames = frames_of(record["sequence changed shape and back 0"])
    assert [staged(f) for f in frames] == [[(w + 1 + 360 + 1) * 8] for w in widths]
    assert [staged(f) for f in frames_of(record["sequence same camera 0"])] == [[(640 + 1 + 360 + 1) * 8], [], []]
