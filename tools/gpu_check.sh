#!/bin/bash
# One GPU-box session: parity tests, smoke, bench, rocprof kernel stats. Outputs -> $OUT/ ($OUT: relative to the repository root, default out)
set -u
O=${OUT:-out}; mkdir -p $O
TAG=${1:-r1}
export TMPDIR=/tmp
echo "== tests"; timeout 900 python -m pytest tests -m gpu -q -p no:cacheprovider 2>&1 | tail -60 | tee $O/${TAG}_tests.log
echo "== smoke"; timeout 300 python __graft_entry__.py --smoke 2>&1 | tail -5 | tee $O/${TAG}_smoke.log
echo "== bench"; timeout 600 python bench.py --full --steps 100 --warmup 10 2> $O/${TAG}_bench.err | tee $O/${TAG}_bench.json
tail -5 $O/${TAG}_bench.err
echo "== rocprof"
( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OLDPWD/$O/${TAG}_prof -- python $OLDPWD/bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --kernel-iters 3 > $OLDPWD/$O/${TAG}_prof_bench.json 2> $OLDPWD/$O/${TAG}_prof.err )
find $O/${TAG}_prof -name "*kernel_stats*" | head; f=$(find $O/${TAG}_prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -25 "$f"
# keep the merged output small: drop the raw trace, keep stats
find $O/${TAG}_prof -type f ! -name "*stats*" -size +1M -delete
