#!/usr/bin/env python3
"""Resource table of the 24 production variants of trace_image_kernel (DIAG = false, not Bounce), from the compiler's own report
(-Rpass-analysis=kernel-resource-usage). No GPU: hipcc cross-compiles.

usage: python tools/trace_resources.py [aic_trace.hip of another checkout ...]
Without arguments: this checkout's csrc/aic_trace.hip. With several sources the tables are printed side by side, first source first
(e.g. the parent commit's file, then this one's)."""
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FIELDS = [("SGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("SGPRs Spill", "s_spill"), ("VGPRs Spill", "v_spill"), ("LDS Size [bytes/block]", "lds")]


def report(source):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", source, "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.split("\n"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = m.group(1) if m.group(1).startswith("_ZN3aic18trace_image_kernel") else None
            if name:
                out[name] = {}
            continue
        if name:
            for label, key in FIELDS:
                m = re.search(r"remark: .*" + re.escape(label) + r": (\d+)", line)
                if m:
                    out[name][key] = int(m.group(1))
    return out


def targs(k):  # <VOL, LMODE, DIAG, BIG, XC> out of the mangled name
    return tuple(int(x) for x in re.search(r"ILb([01])ELi(\d)ELb([01])ELb([01])ELb([01])EE", k).groups())


def main():
    sources = sys.argv[1:] or [os.path.join(ROOT, "all_is_cubes_amd", "csrc", "aic_trace.hip")]
    tables = [report(s) for s in sources]
    for i, s in enumerate(sources):
        print(f"# [{i}] {os.path.relpath(s)}: {len(tables[i])} instantiations of trace_image_kernel")
    keys = [key for _, key in FIELDS]
    print("# <VOL, LMODE, DIAG, BIG, XC>  " + "  ".join(f"{k:>7}" for k in keys) + "   (one line per source)")
    production = sorted((k for k in tables[0] if targs(k)[2] == 0 and targs(k)[1] != 3), key=targs)
    for k in production:
        for i, t in enumerate(tables):
            r = t.get(k, {})
            print(f"{str(targs(k)):<24} [{i}]  " + "  ".join(f"{r.get(key, -1):>7}" for key in keys))
    same = all(t.get(k) == tables[0][k] for k in production for t in tables[1:])
    print(f"# {len(production)} production variants" + ("" if len(tables) < 2 else (": identical in every source" if same else ": the sources differ")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
