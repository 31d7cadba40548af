"""The light updater's queue without a GPU: csrc/aic_light_queue.h (LightGeom, the hashbrown table restated bucket for bucket, LightUpdateQueue) driven by
tests/native/light_queue_check.cpp, a program with its own main built here with -fsanitize=address,undefined. Nothing of it is loaded into Python.

The program checks, at queue widths 0 (first-in-first-out), 8 and 16 (hashbrown's group widths):
  1. set semantics against a plain model, a std::map from cube to priority: seeded random inserts, removes and pops on a 5x4x3 space with a non-zero
     lower corner -- a cube is present once, at the highest priority given to it; pop returns a cube of the highest priority; peek_priority is that
     priority, or 0 when the queue is empty; len is the model's size; a popped or removed cube is gone; clear empties the queue and leaves it usable;
  2. the table's own paths at widths 8 and 16 on a space of 3072 cubes, each proven taken from the table's fields: one priority filled through the
     growths 4 -> 8 -> ... -> 4096 buckets; a churn of erase and insert at constant size that ends in rehash_in_place (growth_left restored, the bucket
     count unchanged); tables of 4 and 8 buckets under a group of 16, and of 4 under a group of 8, reaching the fix_insert_slot line;
  3. the twin: the same program includes oracle/aic_oracle.cpp and feeds the oracle's own LightQueue the same sequences; the popped cubes must be the same,
     element for element, and so must the counts of the paths taken. Exact equality."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SANITIZED = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_header_needs_no_hip(tmp_path):
    """aic_light_queue.h and aic_light_report.h compile with a plain C++17 compiler and the standard library alone."""
    src = tmp_path / "only_std.cpp"
    src.write_text('#include "aic_light_queue.h"\n#include "aic_light_report.h"\nint main() { aic::LightQueue q(1, 16); aic::LightReport r; return (int)q.len + (int)r.cand.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", str(ROOT / "all_is_cubes_amd" / "csrc"), "-c", str(src), "-o", str(tmp_path / "only_std.o")], check=True)


def test_queue_against_model_table_paths_and_the_oracles_twin(tmp_path):
    exe = tmp_path / "light_queue_check"
    build = subprocess.run(SANITIZED + ["-pthread", str(ROOT / "tests" / "native" / "light_queue_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("light queue ok"), run.stdout + run.stderr
