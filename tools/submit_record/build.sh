#!/bin/bash
# Builds one of the programs of this directory from the host sources of one tree:
#   tools/submit_record/build.sh <csrc directory> <output program> [driver.cpp | split_ops_record.cpp | cursor_raycast_record.cpp | listed_ops_record.cpp | light_rays_record.cpp | pick_check.cpp | present_lines_check.cpp] [extra compiler flags]
# (driver.cpp, the frame path's record, when none is named; extra flags e.g. -Xarch_host -fsanitize=address,undefined). Host code only: no device code is
# compiled and nothing of the HIP runtime is linked. The tree's aic_frame.cpp, aic_split_ops.cpp, aic_cursor.cpp, aic_ray_queries.cpp, aic_stale_host.cpp and aic_light_rays_host.cpp
# are added where it has them, and so are aic_exposure_host.cpp and aic_cursor_raycast_host.cpp, which held the ray queries before aic_ray_queries.cpp: a
# tree from before one of them had its own translation unit keeps that code in another, and its record must equal this tree's byte for byte.
#   git archive <parent> all_is_cubes_amd/csrc include | tar -x -C /tmp/parent
#   tools/submit_record/build.sh /tmp/parent/all_is_cubes_amd/csrc /tmp/rec_parent split_ops_record.cpp
#   tools/submit_record/build.sh all_is_cubes_amd/csrc /tmp/rec_new split_ops_record.cpp && cmp <(/tmp/rec_parent) <(/tmp/rec_new)
# The stand-in takes the launchers' declarations from the tree's own headers, so a tree from before one of those headers is built with its own copy of
# this directory (git archive <parent> ... tools/submit_record).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
C="$1"; OUT="$2"; shift 2
MAIN=driver.cpp
case "$1" in *.cpp) MAIN="$1"; shift ;; esac
SRC="$C/aic_abi.cpp"
for part in aic_frame.cpp aic_split_ops.cpp aic_cursor.cpp aic_ray_queries.cpp aic_exposure_host.cpp aic_cursor_raycast_host.cpp aic_stale_host.cpp aic_light_rays_host.cpp; do
    if [ -f "$C/$part" ]; then SRC="$SRC $C/$part"; fi
done
${HIPCC:-/opt/rocm/bin/hipcc} -x hip --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Wall -no-hip-rt -I"$C" -I"$HERE" "$@" $SRC "$HERE/fake_hip.cpp" "$HERE/$MAIN" -o "$OUT"
