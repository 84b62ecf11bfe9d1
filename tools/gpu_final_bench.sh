set -u
export TMPDIR=/tmp
TAG=r03g; P=$PWD; O=${OUT:-out}; mkdir -p $O/$TAG
( time timeout 400 python bench.py --full 2> $O/$TAG/bench.err > $O/$TAG/bench.json ) 2>&1 | tail -3
( cd /tmp && timeout 120 rocprofv3 --kernel-trace --stats --output-format csv -d $P/$O/$TAG/prof -- python $P/bench.py --full --no-cpu-baseline --no-configs --no-sweep > $P/$O/$TAG/prof_bench.json 2> $P/$O/$TAG/prof.err )
f=$(find $O/$TAG/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $O/$TAG/kernel_stats.csv
f=$(find $O/$TAG/prof -name "*kernel_trace.csv" | head -1); [ -n "$f" ] && python tools/trace_by_grid.py "$f" > $O/$TAG/kernel_stats_by_grid.csv
rm -rf $O/$TAG/prof
head -5 $O/$TAG/kernel_stats_by_grid.csv
python - <<PY
import json
d = json.loads(open("$O/$TAG/bench.json").read().strip().splitlines()[-1])
r = d["roofline"]
print(d["value"], d["ms_per_step"], d["config"]["step_frac_of_f32_mfma_peak"], r["kernel"], r["avg_launch_us"], r["frac"], r["traffic"])
s = d.get("sweep") or {}
print({k: v for k, v in s.items() if k in ("gpu_s","cpu_s_extrapolated","gpu_over_cpu_wall_clock","gpu_avg_forgetting")})
print({k: v for k, v in (s.get("pair") or {}).items() if k in ("gpu_s","cpu_s","gpu_accuracies","cpu_accuracies","gpu_over_cpu_wall_clock")})
c = d.get("configs") or {}
for k, v in c.items():
    if isinstance(v, dict) and "ms_per_step" in v: print(k, round(v["ms_per_step"], 3), round(v["frac_of_f32_mfma_peak"], 3))
print(d["cpu_baseline"]["value"], d["config"].get("gpu_over_cpu"))
PY
