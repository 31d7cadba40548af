#!/bin/bash
# Build variants/libaic_hip_<name>.so from the sources of a git revision (default HEAD): the baseline a working-tree change is measured against on the same box
# (profiles/scripts_r06/exp.sh `lib:<name>`). usage: tools/build_ref_variant.sh [name] [rev]
set -e
cd "$(dirname "$0")/.."
NAME=${1:-head}; REV=${2:-HEAD}
D=variants/src_$NAME
rm -rf $D && mkdir -p $D && git archive $REV all_is_cubes_amd/csrc include | tar -x -C $D
C=$D/all_is_cubes_amd/csrc
F="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC"
/opt/rocm/bin/hipcc $F -c $C/aic_trace.hip -o $D/trace.o &
/opt/rocm/bin/hipcc $F -x hip -c $C/aic_abi.cpp -o $D/abi.o &
/opt/rocm/bin/hipcc $F -c $C/aic_light.hip -o $D/light.o &
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -c $C/aic_multi.cpp -o $D/multi.o &
OBJS="$D/trace.o $D/light.o $D/abi.o $D/multi.o"
if [ -f $C/aic_light_host.cpp ]; then  # (revisions from the light host code's own translation unit on; before, aic_abi.cpp included it)
  /opt/rocm/bin/hipcc $F -x hip -c $C/aic_light_host.cpp -o $D/lighthost.o &
  OBJS="$OBJS $D/lighthost.o"
fi
if [ -f $C/aic_frame.cpp ]; then  # (revisions from the frame path's own translation unit on; before, it was part of aic_abi.cpp)
  /opt/rocm/bin/hipcc $F -x hip -c $C/aic_frame.cpp -o $D/frame.o &
  OBJS="$OBJS $D/frame.o"
fi
if [ -f $C/aic_bloom.hip ]; then  # (revisions from the bloom post-process on)
  /opt/rocm/bin/hipcc $F -c $C/aic_bloom.hip -o $D/bloom.o &
  OBJS="$OBJS $D/bloom.o"
fi
if [ -f $C/aic_present.hip ]; then  # (revisions from the presentation post-process on)
  /opt/rocm/bin/hipcc $F -c $C/aic_present.hip -o $D/present.o &
  OBJS="$OBJS $D/present.o"
fi
if [ -f $C/aic_reproject.hip ]; then  # (revisions from the reprojection post-process on)
  /opt/rocm/bin/hipcc $F -c $C/aic_reproject.hip -o $D/reproject.o &
  OBJS="$OBJS $D/reproject.o"
fi
for part in present_lines.hip cursor.cpp pick.hip split_ops.cpp light_chart.cpp light_derived.cpp light_entry.cpp; do  # (the later post-processes, the cursor's host code; from the Split operations' own translation unit on, aic_split_ops.cpp; from the light host code's division by subject on, the chart, compute_derived and the entry points)
  if [ -f $C/aic_$part ]; then
    /opt/rocm/bin/hipcc $F -x hip -c $C/aic_$part -o $D/${part%.*}.o &
    OBJS="$OBJS $D/${part%.*}.o"
  fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -Wl,--no-undefined -o variants/libaic_hip_$NAME.so $OBJS
rm -f $D/*.o
echo "built variants/libaic_hip_$NAME.so from $REV"
