#!/bin/bash
# Build kernel variants locally (hipcc cross-compiles): tools/build_variants.sh "name1:-DFOO=1" "name2:-DBAR=2 -DBAZ"
# Each becomes variants/libaic_hip_<name>.so; tools/exp.sh swaps them in on the GPU box.
# AIC_PATCH=<file>: the variants are built from a copy of csrc/ with that patch applied (e.g. profiles/scripts_r04/experiments_r01_r04.patch, which
# puts the measured-negative experiments of rounds 1-4 -- AIC_SPEC_STEPS, AIC_SHADE_STEP, AIC_PRIO_SHIFT, AIC_HURRY_STEPS, AIC_RAY_MIGRATION, AIC_LDS_PAD,
# AIC_SCHED_SIMPLE, AIC_TRIP_MIN -- back into aic_trace.hip as it stood at the commit that removed them: `git log -- profiles/scripts_r04/experiments_r01_r04.patch`).
# profiles/scripts_r07/retired_switches.patch does the same for the switches whose defaults won and whose other values nobody builds -- AIC_NEWRAY_SKIP_FF,
# AIC_EARLY_APPLY, AIC_OPAQUE_SHORTCUT, AIC_FIRST_LOOKUP, AIC_EXCHANGE, AIC_XCHG_DEPOSIT, AIC_COLD_SCOPE, AIC_FAST_STEPS=0, AIC_FAST_MIN=0 -- on top of the commit
# that retired them (aic_trace.hip and the headers compiled with it, which are copied along: the whole of csrc/ is):
#   AIC_PATCH=profiles/scripts_r07/retired_switches.patch tools/build_variants.sh "ff:-DAIC_NEWRAY_SKIP_FF=1"
set -e
cd "$(dirname "$0")/.."
mkdir -p variants
C=all_is_cubes_amd/csrc
if [ -n "$AIC_PATCH" ]; then
  rm -rf variants/src && mkdir -p variants/src/all_is_cubes_amd && cp -r $C variants/src/all_is_cubes_amd/csrc && cp -r include variants/src/include
  ( cd variants/src && patch -p1 < "../../$AIC_PATCH" )
  C=variants/src/all_is_cubes_amd/csrc
fi
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  ( OBJS="variants/trace_$name.o variants/light_$name.o variants/abi_$name.o variants/lighthost_$name.o variants/multi_$name.o variants/bloom_$name.o"
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -c $C/aic_trace.hip -o variants/trace_$name.o &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -x hip -c $C/aic_abi.cpp -o variants/abi_$name.o &&
    if [ -f $C/aic_frame.cpp ]; then  # (the frame path's own translation unit; an AIC_PATCH tree of an older revision has it inside aic_abi.cpp)
      OBJS="$OBJS variants/frame_$name.o"
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -x hip -c $C/aic_frame.cpp -o variants/frame_$name.o
    fi &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -x hip -c $C/aic_light_host.cpp -o variants/lighthost_$name.o &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -c $C/aic_light.hip -o variants/light_$name.o &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags -x hip -c $C/aic_multi.cpp -o variants/multi_$name.o &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -c $C/aic_bloom.hip -o variants/bloom_$name.o &&
    if [ -f $C/aic_present.hip ]; then  # (the presentation post-process; an AIC_PATCH tree of an older revision has none)
      OBJS="$OBJS variants/present_$name.o"
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -c $C/aic_present.hip -o variants/present_$name.o
    fi &&
    if [ -f $C/aic_reproject.hip ]; then  # (the reprojection post-process; an AIC_PATCH tree of an older revision has none)
      OBJS="$OBJS variants/reproject_$name.o"
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -c $C/aic_reproject.hip -o variants/reproject_$name.o
    fi &&
    for part in present_lines.hip cursor.cpp pick.hip split_ops.cpp light_chart.cpp light_derived.cpp light_entry.cpp; do  # (the later post-processes, the cursor's and the Split operations' host code, the units split off aic_light_host.cpp; an AIC_PATCH tree of an older revision has none)
      if [ -f $C/aic_$part ]; then
        OBJS="$OBJS variants/${part%.*}_$name.o"
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC $flags -x hip -c $C/aic_$part -o variants/${part%.*}_$name.o || exit 1
      fi
    done &&
    # (--no-undefined: an object missing from this list fails here, not when the library is loaded)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -Wl,--no-undefined -o variants/libaic_hip_$name.so $OBJS && rm variants/*_$name.o && echo "built $name" ) &
done
wait
