#!/bin/bash
# diagnostics (WRONG results; -DVRT_DIAG build): what an entry table whose address depends on no loaded value could save at
# most -- VRT_DEBUG_FLAGS=4096 (kDiagDirectTable) reads SOME table at (launch's first slot + slot) x mean entries per slot
# and issues its nine loads ahead of the item's record.  With the pair loop ON the wrong table also sends the gathers to
# sites that are no patch (slower for that reason alone), so the start-up is compared with the pair loop OFF:
# flags 2048 (kDiagNoPairLoop) against 2048 + 4096, alternating (FLAGS overrides the pair); C4 and any bench.py arguments
# usage: tools/direct_table_probe.sh <output file> <repetitions> [bench.py arguments]
set -o pipefail
of=$1; reps=$2; shift 2
mkdir -p $(dirname $of)
lib=${DIAG_LIB:-$PWD/voronoirt_amd/libvrt_hip_diag.so}
echo "# diagnostics build, python bench.py --steps 20 --warmup 5 $*: ms_per_step by VRT_DEBUG_FLAGS (2048: pair loop off; + 4096: table address from blockIdx, loads ahead of the record; wrong results)" >> $of
for rep in $(seq $reps); do
  for flags in ${FLAGS:-2048 6144}; do
    line=$(VRT_LIB_PATH=$lib VRT_DEBUG_FLAGS=$flags timeout -k 10 300 python3 bench.py --gpus 1 --steps 20 --warmup 5 "$@" 2>$of.err | tail -1) || exit 1
    echo "flags $flags $(echo "$line" | python3 -c 'import json,sys; print("%.4f" % json.loads(sys.stdin.read())["ms_per_step"])')" | tee -a $of
  done
done
rm -f $of.err
