#!/usr/bin/env python3
"""Orbit bench.py's atrium in this terminal: the reference's `terminal` graphics mode on the device (aic_render_cells, aic_cells_ansi).

usage: python tools/terminal_view.py [--frames N] [--characters names|shades|split|shapes|braille] [--colors none|256|rgb] [--fps 20]

Keys (as the reference binds them, terminal.rs:222-236): m cycles the character mode, n the colour mode; q or Ctrl-C quits. Without a terminal on stdin
(a pipe) the keys are not read and --frames bounds the run. The drawing area is the terminal's size less one row for the status line. A demo: no test
runs it."""
import argparse
import math
import os
import shutil
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHARACTERS = ("names", "shades", "split", "shapes", "braille")
COLORS = ("none", "256", "rgb")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=0, help="stop after this many frames (0: until q)")
    ap.add_argument("--characters", choices=CHARACTERS, default="split")
    ap.add_argument("--colors", choices=COLORS, default="256")
    ap.add_argument("--fps", type=float, default=20.0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import oracle
    from all_is_cubes_amd import abi

    characters, colors = CHARACTERS.index(args.characters), COLORS.index(args.colors)
    sp, _, eye, target, vd, _ = bench.build_workload("atrium")
    names = ([("#" if b.name in ("", "#") else b.name[0]) for b in sp.blocks], None)
    radius = math.hypot(eye[0] - target[0], eye[2] - target[2])
    interactive = sys.stdin.isatty()
    restore = None
    if interactive:
        import termios
        import tty

        restore = termios.tcgetattr(sys.stdin.fileno())
        tty.setcbreak(sys.stdin.fileno())
    out = sys.stdout.buffer
    try:
        with abi.Context(0) as ctx:
            ctx.upload_space(abi.LAYER_WORLD, sp)
            ctx.set_options(abi.LAYER_WORLD, abi.make_options(view_distance=vd))
            out.write(b"\x1b[2J")
            frame = 0
            while not args.frames or frame < args.frames:
                t0 = time.perf_counter()
                size = shutil.get_terminal_size((80, 24))
                cols, rows = max(size.columns, 1), max(size.lines - 1, 1)
                (w, h), nominal = abi.cells_geometry(cols, rows, characters)
                angle = frame * 0.03
                at = (target[0] + radius * math.sin(angle), eye[1], target[2] + radius * math.cos(angle))
                _, _, inv = oracle.camera_matrices(90.0, vd, nominal[0] / nominal[1], oracle.look_at_y_up(at, target), at)
                cells, fi, ci = ctx.render_cells(ctx.make_frame(w, h, world_inv=inv), cols, rows, characters, colors)
                out.write(abi.cells_ansi(cells, names, None, in_rect=True, origin=(0, 0)))
                status = f" {CHARACTERS[characters]} / {COLORS[colors]}  {w}x{h} rays  trace {fi.kernel_ms:.2f} ms  cells {ci.kernel_ms:.3f} ms  [m] [n] [q] "
                out.write(f"\x1b[{rows + 1};1H\x1b[0m{status[:cols]}\x1b[K".encode())
                out.flush()
                frame += 1
                if interactive:
                    import select

                    wait = max(0.0, 1.0 / args.fps - (time.perf_counter() - t0))
                    if select.select([sys.stdin], [], [], wait)[0]:
                        key = sys.stdin.read(1)
                        if key in ("q", "\x03", "\x04"):
                            break
                        if key == "m":
                            characters = (characters + 1) % 5
                            out.write(b"\x1b[2J")
                        elif key == "n":
                            colors = (colors + 1) % 3
    finally:
        out.write(b"\x1b[0m\x1b[?25h\r\n")
        out.flush()
        if restore is not None:
            import termios

            termios.tcsetattr(sys.stdin.fileno(), termios.TCSADRAIN, restore)


if __name__ == "__main__":
    main()
