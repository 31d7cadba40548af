#!/usr/bin/env python3
"""What a terminal frame costs, in ONE GPU command (profiles/terminal_cells.txt).

usage: python tools/cells_timing.py [--rounds 60] [--out profiles/terminal_cells.txt]

bench.py's atrium with its light, uploaded once, seen by the bench's camera in a terminal of 200 x 60 cells (nominal aspect 200 * 0.5 / 60). For each
CharacterMode (colours TwoFiftySix, the reference's default) two legs, each a blocking call timed with the host's wall clock around it, interleaved round
by round after 10 rounds of warm-up:
  * cells:  aic_render_cells into host memory -- the trace, the cells kernel, 12 bytes a cell read back; its cells kernel's kernel_ms (HIP events) beside;
  * parent: the path to the same information without the feature -- an AIC_FRAME_OUT_LINEAR | AIC_FRAME_AUX frame of the same size into host memory and
            aic_read_aux of its records: 16 + 56 bytes a pixel read back. The host's patch rule that would follow is NOT timed.
Median, 10th and 90th percentile over the rounds, and the bytes that cross the bus either way. No threshold rests on these figures."""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLS, ROWS = 200, 60
NAMES = ("Names", "Shades", "Split", "Shapes", "Braille")


def measure(rounds, say):
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench
    import oracle
    from all_is_cubes_amd import abi

    sp, _, eye, target, vd, _ = bench.build_workload("atrium")
    _, _, inv = oracle.camera_matrices(90.0, vd, (COLS * 0.5) / (ROWS * 1.0), oracle.look_at_y_up(eye, target), eye)
    pct = lambda v: tuple(float(np.percentile(np.array(v), q)) for q in (50, 10, 90))  # noqa: E731
    with abi.Context(0) as ctx:
        ctx.upload_space(abi.LAYER_WORLD, sp)
        ctx.set_options(abi.LAYER_WORLD, abi.make_options(view_distance=vd))
        say(f"device: {ctx.device_name}; atrium, {COLS} x {ROWS} cells, colours TwoFiftySix, {rounds} interleaved rounds after 10 of warm-up; milliseconds: median (p10 .. p90)")
        for characters in range(5):
            (w, h), _ = abi.cells_geometry(COLS, ROWS, characters)
            cells_ms, kernel_ms, parent_ms = [], [], []
            for r in range(rounds + 10):
                t0 = time.perf_counter()
                cells, fi, ci = ctx.render_cells(ctx.make_frame(w, h, world_inv=inv), COLS, ROWS, characters, abi.CELLS_COLOR_256)
                t1 = time.perf_counter()
                ctx.render(ctx.make_frame(w, h, world_inv=inv, flags=abi.FRAME_OUT_LINEAR), want_aux=True)
                t2 = time.perf_counter()
                if r >= 10:
                    cells_ms.append((t1 - t0) * 1e3)
                    kernel_ms.append(ci.kernel_ms)
                    parent_ms.append((t2 - t1) * 1e3)
            a, k, b = pct(cells_ms), pct(kernel_ms), pct(parent_ms)
            say(f"{NAMES[characters]:8s} {w:4d} x {h:3d} rays | aic_render_cells {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}), cells kernel {k[0]:.4f} ({k[1]:.4f} .. {k[2]:.4f}), "
                f"{COLS * ROWS * 12} bytes back | linear + aux frame and aic_read_aux {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}), {w * h * 72} bytes back")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    measure(args.rounds, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
