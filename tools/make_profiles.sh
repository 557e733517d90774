#!/bin/bash
# Produces the rocprofv3 evidence committed under profiles/: kernel-trace stats of the default C4
# bench command and the PMC passes of ONE step (separate runs per counter group, no tracing
# alongside), then the bench lines with --full.  Run on an MI355X:  bash tools/make_profiles.sh <round-tag>
# (results under $VRT_RESULTS, default results/; tools/summarise_profiles.py copies the summaries into profiles/<round>/;
# bench.py quotes roofline.traffic only once that summary carries the library's digest, so the committed
# bench_default.json is a `python bench.py --full > $VRT_RESULTS/<tag>_bench_default.json` run AFTER the summary
# step, followed by the summary step once more)
tag=${1:-r2}
res=${VRT_RESULTS:-results}; mkdir -p $res
bash tools/prof_kernels.sh ${tag}_default > $res/${tag}_kernel_stats.txt 2>&1 || { tail -5 $res/${tag}_kernel_stats.txt; exit 1; }
PMC_EXTRA="TCC_EA0_RDREQ_DRAM_sum TCC_EA0_WRREQ_DRAM_sum" bash tools/prof_pmc.sh ${tag}_default > $res/${tag}_pmc.txt 2>&1 || { tail -5 $res/${tag}_pmc.txt; exit 1; }
python3 bench.py --full > $res/${tag}_bench_default.json 2> $res/${tag}_bench_default.err || exit 1
python3 bench.py --full --workload C3 --no-secondary > $res/${tag}_bench_c3.json 2>/dev/null || exit 1
python3 bench.py --full --workload C5 --dtype f32 --steps 3 --warmup 1 --no-secondary > $res/${tag}_bench_c5_f32.json 2>/dev/null || exit 1
python3 tools/real_grid_check.py 1000000 24 > $res/${tag}_real_grid_1m.txt 2>&1 || exit 1
# kernel trace of the same on the default path only (1 M density-stratified, tessellated sites x 12 x 24 wavelengths)
rm -rf $res/prof_${tag}_real1m; mkdir -p $res/prof_${tag}_real1m
TMPDIR=/tmp REAL_GRID_DEFAULT_ONLY=1 rocprofv3 --kernel-trace --stats --output-format csv -d $res/prof_${tag}_real1m -o p -- python3 tools/real_grid_check.py 1000000 24 > $res/prof_${tag}_real1m/run.log 2>&1 || exit 1
for w in C3 C5; do
  rm -rf $res/prof_${tag}_$w; mkdir -p $res/prof_${tag}_$w
  extra=""; [ $w = C5 ] && extra="--dtype f32"
  TMPDIR=/tmp rocprofv3 --kernel-trace --stats --output-format csv -d $res/prof_${tag}_$w -o p -- python3 bench.py --workload $w $extra --steps 3 --warmup 1 --no-cpu-baseline --no-secondary --no-critical-path > $res/prof_${tag}_$w/bench.log 2>&1 || exit 1
done
cat $res/${tag}_kernel_stats.txt $res/${tag}_pmc.txt
