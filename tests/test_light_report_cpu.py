"""The light updater's changed-cube report without a GPU: csrc/aic_light_report.h (what aic_light_changed_count / _take answer from) driven by
tests/native/light_report_check.cpp, a program with its own main built here with -fsanitize=address,undefined. Nothing of it is loaded into Python.

The program drives the report as the library does, on volumes of 336 and 125 texels, beside a brute-force model kept as two whole volumes, and checks:
a cube is reported if and only if the updater wrote it since the last take and its texel differs from the baseline; the list is ascending, in the cand
mode and in the cand_all mode (a full relight); take() empties the report; the caller's own texels are never reported; a re-read of the mirror keeps a
pending report whose texel it did not move -- with reread_own false -- and every pending report the device still differs in -- with reread_own true
--, and the program counts the reports that only the second rule keeps; a re-read under another serial or another size starts afresh."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_report_against_two_whole_volumes(tmp_path):
    exe = tmp_path / "light_report_check"
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            str(ROOT / "tests" / "native" / "light_report_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("light report ok"), run.stdout + run.stderr
