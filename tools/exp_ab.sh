#!/bin/bash
# A/B of builds of the library on one box, alternating: bash tools/exp_ab.sh <rounds> <name under tksm_amd/> <name> ...
cd "$(dirname "$0")/.."
set -o pipefail
export GPU_MAX_HW_QUEUES=16
N=$1; shift
out=gpurun_out/exp_ab.log
: > $out
B="python bench.py --full --steps 12 --warmup 2 --no-cpu-baseline --no-e2e --no-side-legs"
# (a run that fails or hangs ends the comparison: nothing more is started on the device)
one() { echo -n "$1: " >> $out; TKSMSEQ_LIB=$1 timeout -k 10 300 $B 2>/dev/null | python -c "
import sys,json
d=json.loads(sys.stdin.readline())
x=d.get('roofline',{}).get('exclusive_ms_per_step') or {}
print(round(d['value']/1e6,3), 'M reads/s', round(d['ms_per_step'],2), 'ms/step; exclusive', {k: round(v,2) for k,v in x.items()})" >> $out; }
for i in $(seq $N); do for l in "$@"; do one $l || { echo "$l: run failed" >> $out; cat $out; exit 1; }; done; done
cat $out
