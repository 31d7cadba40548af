"""aic_present_split_lines' host side without a GPU: tools/submit_record/present_lines_check.cpp drives csrc/aic_split_ops.cpp against the recording fake of the
HIP runtime and of the kernel launchers -- every rejection queues and allocates nothing, a call without lines makes exactly aic_present_split's calls, the
line scratch grows and is released, failing runtime calls leave the context usable -- and exits 0 when all of it holds. The program has its own main and
is built here with -fsanitize=address,undefined: host code only, nothing of it is loaded into Python."""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_present_lines_check_passes_under_the_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_present_lines_check_"), "present_lines_check")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "present_lines_check.cpp", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"], check=True, capture_output=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert " 0 of " in run.stderr and "LEAK" not in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    lines = [line for line in run.stdout.split("\n") if not line.startswith("  ")]  # (a launcher's arguments follow its name, indented)
    # a lines call: S stored, the line pass, then the presentation of S'
    at = [i for i, line in enumerate(lines) if line.startswith("launch_present_lines")]
    assert len(at) >= 10
    for i in at:
        assert lines[i - 1] == "launch_present_scene" and lines[i + 1] == "launch_present"
    assert sum(line == "launch_present_scene" for line in lines) == len(at)
    # where the program announces whether the keys are cleared, the launch says the same
    announced = [i for i, line in enumerate(lines) if line.startswith("#")]
    assert len(announced) >= 9
    for i in announced:
        want = lines[i].rsplit(" ", 2)[-2:]
        launch = next(line for line in lines[i:] if line.startswith("launch_present_lines"))
        assert want[0] == "clear_keys" and f" clear_keys {want[1]} " in launch, (lines[i], launch)
    assert any(line.startswith("hipFree") for line in lines)
