#!/bin/bash
# Profile of one build of the library, for a before / after pair: the kernel-trace runs of tools/profile_round.sh (three contexts, one context) and the SQ and TCC
# passes of tools/pmc_round3.sh, each a run of its own, for one library; every step under its own time limit, chained
# usage (GPU box, repo root): bash tools/profile_lib.sh <library under tksm_amd/> <output directory>
set -o pipefail
export TKSMSEQ_LIB=$1
R=$PWD; mkdir -p "$2"; out=$(cd "$2" && pwd)
cd /tmp && export TMPDIR=/tmp
export GPU_MAX_HW_QUEUES=16
Bn=1310720
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats -- python $R/bench.py --full --no-cpu-baseline --no-e2e --no-side-legs > $out/bench_under_rocprof.json 2> $out/stats.err && echo stats >> $out/progress.log &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats1 -- python $R/bench.py --full --no-cpu-baseline --no-e2e --no-side-legs --pipeline 1 --steps 4 > $out/bench_single_ctx_under_rocprof.json 2> $out/stats1.err && echo stats1 >> $out/progress.log &&
timeout -k 10 240 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES --output-format csv -d $out/sq -- python $R/tools/quick_stage_times.py $Bn > $out/sq.log 2>&1 && echo sq >> $out/progress.log &&
timeout -k 10 240 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum GRBM_GUI_ACTIVE --output-format csv -d $out/tcc -- python $R/tools/quick_stage_times.py $Bn > $out/tcc.log 2>&1 && echo tcc >> $out/progress.log
rc=$?
cd $R
if [ $rc -ne 0 ]; then echo "a profile step failed rc=$rc"; cat $out/progress.log; tail -5 $out/*.err $out/*.log; exit $rc; fi
for p in sq tcc; do python tools/pmc_kernels.py $out/$p > $out/$p.txt 2>&1; done
cp $out/stats/*/*kernel_stats.csv $out/kernel_stats.csv
cp $out/stats1/*/*kernel_stats.csv $out/single_ctx_kernel_stats.csv
rm -rf $out/stats $out/stats1 $out/sq $out/tcc
grep -h "k_loop" $out/kernel_stats.csv $out/single_ctx_kernel_stats.csv $out/sq.txt $out/tcc.txt | cut -c1-400
cat $out/bench_under_rocprof.json | cut -c1-300
