#!/bin/bash
# diagnostics: A/B of two builds of the library in one session (profiles/edges): the parent commit's library (PARENT_LIB,
# default voronoirt_amd/libvrt_hip_parent.so) against this one, alternating, with the driver's own command and any
# bench.py arguments (tools/ab_libs.sh runs a fixed set of workloads with the lean flags instead)
# usage: tools/edges_ab.sh <output file> <repetitions> [bench.py arguments, e.g. --workload C3]
set -o pipefail
of=$1; reps=$2; shift 2
mkdir -p $(dirname $of)
P=${PARENT_LIB:-$PWD/voronoirt_amd/libvrt_hip_parent.so}; B=$PWD/voronoirt_amd/libvrt_hip.so
echo "# python bench.py --gpus 1 --steps 20 --warmup 5 $*: ms_per_step; parent = the parent commit's library, branch = this library" >> $of
for rep in $(seq $reps); do
  for cfg in parent branch; do
    case $cfg in parent) lib=$P;; branch) lib=$B;; esac
    line=$(VRT_LIB_PATH=$lib timeout -k 10 400 python3 bench.py --gpus 1 --steps 20 --warmup 5 "$@" 2>/dev/null | tail -1) || exit 1
    echo "$cfg $(echo "$line" | python3 -c 'import json,sys; print("%.4f" % json.loads(sys.stdin.read())["ms_per_step"])')" | tee -a $of
  done
done
