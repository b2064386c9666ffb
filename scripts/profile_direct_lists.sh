#!/bin/bash
# Where a change's gain is (direct lists, PERFLOG row 178; direct resolve,
# row 179), for A = libmcpt_a.so, the parent commit's build
# (scripts/build_base.sh libmcpt_a.so), and B = libmcpt.so: a kernel trace of
# one C2 frame on one stream (extend and shade per bounce,
# scripts/wf_bounce_times.py), then, in runs of their own with no tracing
# alongside, SQ_INSTS_VALU per kernel class (scripts/valu_by_class.py); then the
# refill threshold re-swept on B, two alternated rounds.  Any failing step ends
# the script.  Output under $OUT.
set -e -o pipefail
R=$PWD
O=${OUT:-$R/build/prof_direct}; mkdir -p $O
L=$R/montecarlopathtracer_amd/lib
export TMPDIR=/tmp
for side in A B; do
  lib=libmcpt.so; [ $side = A ] && lib=libmcpt_a.so
  (cd /tmp && MCPT_LIB_PATH=$L/$lib timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $O/kt_$side -o run -- \
     python3 $R/bench.py --gpus 1 --steps 1 --warmup 0 --wf-streams 1 > $O/kt_$side.log 2>&1)
  python3 scripts/wf_bounce_times.py $O/kt_$side | tee $O/bounce_times_$side.txt
done
for side in A B; do
  lib=libmcpt.so; [ $side = A ] && lib=libmcpt_a.so
  (cd /tmp && MCPT_LIB_PATH=$L/$lib timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d $O/pmc_$side -o run -- \
     python3 $R/bench.py --pmc-child > $O/pmc_$side.log 2>&1)
  python3 scripts/valu_by_class.py $O/pmc_$side | tee $O/insts_valu_$side.txt
done
for r in 1 2; do
  vals="8 16 24 32"; [ $r = 2 ] && vals="32 24 16 8"
  for v in $vals; do
    timeout -k 10 240 python bench.py --gpus 1 --steps 10 --warmup 3 --set wf_refill=$v > $O/refill_${v}_$r.log 2>&1
    echo "round $r wf_refill=$v: $(grep -o '"ms_per_step": [0-9.]*' $O/refill_${v}_$r.log)" | tee -a $O/refill_sweep.txt
  done
done
