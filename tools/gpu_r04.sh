#!/bin/bash
# r04: GPU parity tests, then the profile recipe, then a full-mask-mode bench for comparison.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${MRTS_OUT:-out}; mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1 || exit $?
bash tools/gpu_profile.sh r04 || exit $?
timeout -k 10 300 python bench.py --full --mask-mode full --no-cpu-baseline > $OUT/r04/bench_full.json 2> $OUT/r04/bench_full.err || exit $?
