#!/bin/bash
# A/B on ONE box (boxes differ by a few percent): bench.py with the library in the tree (B) and with .ab/libA.so (A), alternating.
# VARIANTS names the rotation: B is the tree's library, any other name X is .ab/libX.so.
# usage (on the GPU box): [PAIRS=3] [VARIANTS="A B"] bash tools/ab_bench.sh [bench args]
# A run that does not end with a result line stops the rotation (nothing more is started on a GPU that may have faulted).
OUT=${OUT:-bench_out}
PAIRS=${PAIRS:-3}
mkdir -p "$OUT"
VARIANTS=${VARIANTS:-A B}
for k in $(seq 1 "$PAIRS"); do
  for v in $VARIANTS; do
    if [ $v = B ]; then unset SPCBPT_LIB; else export SPCBPT_LIB=$PWD/.ab/lib$v.so; fi
    timeout -k 10 300 python bench.py --full --no-cpu-baseline --fast-math-line 0 "$@" 2>"$OUT/ab_err_$v.log" | python -c "
import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['value'], 'Mpaths/s', d['ms_per_step'], 'ms/step, kernel', d['roofline']['kernel_ms'])" || { tail -5 "$OUT/ab_err_$v.log"; exit 1; }
  done
done
