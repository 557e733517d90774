#!/bin/bash
# diagnostics: the edges of the per-layer patch launches of C4 with one library (profiles/edges/INDEX.md):
#   the kernel boundary (tools/launch_gaps.py over a rocprofv3 kernel trace) and, with the -DVRT_DIAG build of the same
#   sources, the step with the pair loop switched off (VRT_DEBUG_FLAGS=2048: WRONG results, start-up and drain alone)
# usage: tools/prof_edges.sh <library> <its diagnostics build> <output directory>
set -o pipefail
lib=$1; diag=$2; out=$3
mkdir -p $out/trace
export TMPDIR=/tmp
lean="--no-cpu-baseline --no-secondary --no-critical-path"
VRT_LIB_PATH=$lib timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -o p -- \
    python3 bench.py --steps 3 --warmup 1 $lean > $out/trace_bench.log 2>&1 || exit 1
f=$(find $out/trace -name '*kernel_trace.csv' | head -1)
python3 tools/launch_gaps.py "$f" k_patch_ | tee $out/gaps.txt || exit 1
for flags in 0 2048; do
    line=$(VRT_LIB_PATH=$diag VRT_DEBUG_FLAGS=$flags timeout -k 10 200 python3 bench.py --steps 5 --warmup 2 $lean 2>$out/diag_$flags.err | tail -1) || exit 1
    echo "diag flags $flags $(echo "$line" | python3 -c 'import json,sys; print("ms_per_step %.3f" % json.loads(sys.stdin.read())["ms_per_step"])')" | tee -a $out/gaps.txt
done
rm -rf $out/trace
