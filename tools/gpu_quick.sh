#!/bin/bash
# parity subset + bench line (no cpu baseline): the inner loop of a tuning session
set -u
O=${OUT:-out}; mkdir -p $O; export TMPDIR=/tmp
timeout 900 python -m pytest tests/test_gpu_parity.py -q -x -p no:cacheprovider ${1:+-k "$1"} 2>&1 | tail -4
timeout 300 python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline 2>/dev/null | tee $O/quick.json | cut -c1-330
