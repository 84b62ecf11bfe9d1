#!/bin/bash
# bench + rocprofv3 kernel stats of the same command. Outputs -> $OUT/<tag>_* ($OUT: relative to the repository root, default out)
set -u
TAG=${1:-r2}
O=${OUT:-out}; mkdir -p $(dirname $O/$TAG)
export TMPDIR=/tmp
timeout 600 python bench.py --full --steps 100 --warmup 10 ${2:-} 2> $O/${TAG}_bench.err > $O/${TAG}_bench.json
tail -3 $O/${TAG}_bench.err
( cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OLDPWD/$O/${TAG}_prof -- python $OLDPWD/bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --no-configs --no-sweep --kernel-iters 3 > $OLDPWD/$O/${TAG}_prof_bench.json 2> $OLDPWD/$O/${TAG}_prof.err )
f=$(find $O/${TAG}_prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $O/${TAG}_kernel_stats.csv && head -30 "$f" | cut -c1-200
find $O/${TAG}_prof -type f ! -name "*stats*" -size +1M -delete
