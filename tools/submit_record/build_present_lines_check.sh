#!/bin/bash
# Builds present_lines_check (the host side of aic_present_split_lines and aic_cursor_wireframe against the recording fake) from the host sources of one tree:
#   tools/submit_record/build_present_lines_check.sh <csrc directory> <output program> [extra compiler flags]
# e.g. -Xarch_host -fsanitize=address,undefined -- host code only, as build.sh: no device code is compiled and nothing of the HIP runtime is linked.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
C="$1"; OUT="$2"; shift 2
${HIPCC:-/opt/rocm/bin/hipcc} -x hip --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Wall -no-hip-rt -I"$C" -I"$HERE" "$@" "$C/aic_abi.cpp" "$C/aic_frame.cpp" "$C/aic_cursor.cpp" "$HERE/fake_hip.cpp" "$HERE/present_lines_check.cpp" -o "$OUT"
