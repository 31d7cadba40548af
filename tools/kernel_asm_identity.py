"""Per-kernel comparison of two device listings: has a change that was meant to leave the code object alone done so?
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall --cuda-device-only -S aic_trace.hip -o new.s   (the Makefile's flags; the same for the other tree)
  python tools/kernel_asm_identity.py parent.s new.s      (exit 0: at least one kernel, and every kernel identical)
Kernels are matched by symbol, so their order in the file does not matter. A kernel's text runs from its `.protected <sym> ; -- Begin function` line
(`.globl <sym> ; -- Begin function` for a kernel in an anonymous namespace) through its instructions, its .amdhsa_kernel descriptor and the `; Kernel info:` resource comments. The function index in .LBB<n>_ / .Lfunc_end<n> labels
is normalised (it only counts the functions ahead of this one in the file)."""
import re, sys
def kernels(path):
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"\s*\.(protected|globl)\s+\S+\s*; -- Begin function", l)]
    end_all = next(i for i, l in enumerate(lines) if ".AMDGPU.gpr_maximums" in l)
    out = {}
    for a, b in zip(starts, starts[1:] + [end_all]):
        chunk = lines[a:b]
        while chunk and re.match(r"\s*\.(text|section\s+\.text)", chunk[-1]): chunk.pop()
        name = lines[a].split()[1]
        body = "\n".join(chunk)
        assert ".amdhsa_kernel " + name in body and "; Kernel info:" in body, name
        body = re.sub(r"\.LBB\d+_", ".LBB#_", body)
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end#", body)
        out[name] = body
    return out
a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
same = [k for k in a if k in b and a[k] == b[k]]
for k in a:
    if k not in b: print("missing:", k)
    elif a[k] != b[k]:
        la, lb = a[k].split("\n"), b[k].split("\n")
        d = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
        print("DIFFERS:", k, len(la), len(lb), "first at", d, "|", la[d] if d is not None else "", "|", lb[d] if d is not None else "")
for k in b:
    if k not in a: print("extra:", k)
n_trace = sum("trace_image_kernel" in k for k in a)
print(f"{len(a)} kernels ({n_trace} trace_image_kernel instantiations) in {sys.argv[1]}, {len(b)} in {sys.argv[2]}; identical: {len(same)} / {len(a)}")
if not a: print("no kernel found in", sys.argv[1])
sys.exit(0 if a and len(same) == len(a) == len(b) else 1)
