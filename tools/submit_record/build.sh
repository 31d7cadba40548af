#!/bin/bash
# Builds the submit-record program from the host sources of one tree: tools/submit_record/build.sh <csrc directory> <output program> [extra compiler flags]
# (e.g. -Xarch_host -fsanitize=address,undefined). Host code only: no device code is compiled and nothing of the HIP runtime is linked. A tree from before the
# frame path had its own translation unit has no aic_frame.cpp; its record must equal this tree's byte for byte. The stand-in takes the launchers'
# declarations from the tree's aic_launch.h, so a tree from before that header is built with its own copy of this directory:
#   git archive <parent> all_is_cubes_amd/csrc include tools/submit_record | tar -x -C /tmp/parent
#   /tmp/parent/tools/submit_record/build.sh /tmp/parent/all_is_cubes_amd/csrc /tmp/rec_parent && tools/submit_record/build.sh all_is_cubes_amd/csrc /tmp/rec_new
#   cmp <(/tmp/rec_parent) <(/tmp/rec_new)
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
C="$1"; OUT="$2"; shift 2
SRC="$C/aic_abi.cpp"
if [ -f "$C/aic_frame.cpp" ]; then SRC="$SRC $C/aic_frame.cpp"; fi
${HIPCC:-/opt/rocm/bin/hipcc} -x hip --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Wall -no-hip-rt -I"$C" -I"$HERE" "$@" $SRC "$HERE/fake_hip.cpp" "$HERE/driver.cpp" -o "$OUT"
