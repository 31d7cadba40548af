"""aic_pick_pixels' host side without a GPU: tools/submit_record/pick_check.cpp drives csrc/aic_split_ops.cpp against the recording fake of the HIP runtime
and of the kernel launchers -- every rejection the header lists, the state aic_reproject_split keeps for the call, what a good call allocates and copies --
and exits 0 when all of it holds. (The same program is what a sanitizer build runs: tools/submit_record/build.sh says how.)"""
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_pick_check_passes():
    exe = os.path.join(tempfile.mkdtemp(prefix="aic_pick_check_"), "pick_check")
    subprocess.run(["bash", str(ROOT / "tools" / "submit_record" / "build.sh"), str(ROOT / "all_is_cubes_amd" / "csrc"), exe, "pick_check.cpp"], check=True, capture_output=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert " 0 of " in run.stderr and "LEAK" not in run.stdout
    lines = [line for line in run.stdout.split("\n") if not line.startswith("  ")]  # (a launcher's arguments follow its name, indented)
    assert sum(line == "launch_pick" for line in lines) >= 4
    assert any(line.startswith("hipFree") for line in lines)
