#!/bin/bash
# Interleaved bench.py runs under several prebuilt libraries, on one box in one session:
#   profiles/scripts_r07/ab_libs.sh OUTDIR ROUNDS "parent new" "c2|--no-cpu-baseline --no-extras --min-seconds 3" "s256|--workload s256 ..." ...
# For every round, every configuration ("name|bench arguments") and every library name L it copies variants/libaic_hip_L.so over the package's library, runs
# bench.py --gpus 1 under a time limit, keeps the JSON line as OUTDIR/<name>_<L>_<round>.json and prints its figures. It stops at the first run that fails and puts
# variants/libaic_hip_$DEFAULT_LIB.so (default: the last library named) back in place when it ends. Libraries: the tree's own build copied to variants/, a parent
# commit's build of csrc/, tools/build_variants.sh for -D variants. profiles/open_cubes_timing.txt is such a session.
set -o pipefail
cd "$(dirname "$0")/../.."
O=$1; ROUNDS=$2; LIBS=$3; shift 3
DEFAULT_LIB=${DEFAULT_LIB:-${LIBS##* }}
mkdir -p $O
restore() { cp variants/libaic_hip_$DEFAULT_LIB.so all_is_cubes_amd/libaic_hip.so; }
for r in $(seq 1 $ROUNDS); do
  for cfg in "$@"; do
    name=${cfg%%|*}; args=${cfg#*|}
    for lib in $LIBS; do
      cp variants/libaic_hip_$lib.so all_is_cubes_amd/libaic_hip.so || exit 1
      f=$O/${name}_${lib}_$r.json
      timeout -k 10 240 python bench.py --gpus 1 $args > $f.full 2> $f.err; rc=$?
      if [ $rc != 0 ]; then echo "FAILED rc $rc: $name $lib round $r"; tail -5 $f.err; restore; exit $rc; fi
      tail -1 $f.full > $f
      python profiles/scripts_r07/ab_line.py "$f" "$name" "$lib" "$r"
    done
  done
done
restore
