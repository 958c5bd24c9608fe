#!/bin/bash
# Same-box A/B of two library builds (interleaved runs): bash tools/ab_bench.sh <tag> <prev.so> "<configs>" [reps]
# Results: $MRTS_OUT/<tag>/ (default out/<tag>/): <config>_{prev,new}_<rep>.json
set -o pipefail
TAG=$1; PREV=$2; CFGS=${3:-c3}; REPS=${4:-2}
OUT=${MRTS_OUT:-out}/$TAG; mkdir -p $OUT
A="--full --no-cpu-baseline --no-other-configs ${AB_ARGS:---no-compare}"
for i in $(seq 1 $REPS); do
  for c in $CFGS; do
    MRTS_LIB_PATH=$PREV timeout -k 10 300 python bench.py --config $c $A > $OUT/${c}_prev_$i.json 2>> $OUT/err.log || exit $?
    timeout -k 10 300 python bench.py --config $c $A > $OUT/${c}_new_$i.json 2>> $OUT/err.log || exit $?
  done
done
