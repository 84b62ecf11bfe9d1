"""clhip_lwf_loss (one block, one thread per row) against clhip_lwf_loss_wide (one wave per row over the GPU + a one-block
sum) at N = 200 rows, T = 2, with distillation, on
  10x20     [20] * 10                                   the 10-task Tiny-ImageNet split (what clhip_lwf_loss was written for)
  recogseq  [102, 67, 200, 196, 100, 11, 52, 11]        739 columns
  32x5      [5] * 32                                    the longest sequence clhip_lwf_loss takes
  40x5      [5] * 40                                    the wide kernel alone
HIP-event timed in one process: every round times --calls back-to-back calls of the narrow entry, then of the wide entry
(alternating inside the round), per layout; reported per call: the median over the rounds, min, max and the relative
spread (max - min) / median, which is what a difference between the two has to exceed to count.  --profile adds ONE run of
this script under `rocprofv3 --kernel-trace --stats` in a child process of its own (tracing slows the host: the event
times above are taken with the profiler off) and reports the average kernel durations per layout from the trace.
python tools/lwf_loss_bench.py [--rounds 20] [--calls 50] [--warmup 3] [--profile] [--out profiles/lwf_wide_loss.json]"""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, LAM = 200, 2.0, 1.0
LAYOUTS = [("10x20", [20] * 10, True), ("recogseq", [102, 67, 200, 196, 100, 11, 52, 11], True), ("32x5", [5] * 32, True),
           ("40x5", [5] * 40, False)]           # name, head sizes, clhip_lwf_loss takes it
KERNELS = ("lwf_loss_kernel", "lwf_wide_rows_kernel", "lwf_wide_sum_kernel")


def make_calls(L, torch, sizes):
    width, old = sum(sizes), sum(sizes[:-1])
    gen = torch.Generator().manual_seed(7)
    z = (torch.randn((N, width), generator=gen) * 3).cuda()
    t = (torch.randn((N, old), generator=gen) * 3).cuda()
    y = torch.randint(0, sizes[-1], (N,), generator=gen).cuda()
    dz = torch.zeros((N, width), device="cuda")
    loss2 = torch.zeros(2, device="cuda")
    hs = (C.c_int * len(sizes))(*sizes)
    need = L.clhip_lwf_loss_wide_ws(len(sizes), N)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    keep = (z, t, y, dz, loss2, hs, ws)
    args = (z.data_ptr(), y.data_ptr(), t.data_ptr(), hs, len(sizes), N, width, old, T, LAM, 1, dz.data_ptr(), loss2.data_ptr(), None)
    stream = torch.cuda.current_stream().cuda_stream

    def narrow():
        rc = L.clhip_lwf_loss(*args, stream)
        assert rc == 0, rc

    def wide():
        rc = L.clhip_lwf_loss_wide(*args, ws.data_ptr(), need, stream)
        assert rc == 0, rc
    return narrow, wide, keep


def timed(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def summary(v):
    med = statistics.median(v)
    return {"median_us": med, "min_us": min(v), "max_us": max(v), "spread": (max(v) - min(v)) / med}


def trace_times(out_dir):
    """Average kernel durations per layout from the kernel trace: the child runs the layouts in order, per layout the
    narrow calls (where the kernel takes the layout) and then the wide calls, so the trace splits by position."""
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        return {"error": "no kernel trace written"}
    rows = []
    for r in csv.DictReader(open(paths[0])):
        name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if name:
            rows.append((int(r["Start_Timestamp"]), name, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    return [(name, ns) for _, name, ns in rows]


def profile_child(a):
    """ONE run under rocprofv3 --kernel-trace --stats; the program itself goes after `--`."""
    with tempfile.TemporaryDirectory() as d:
        calls = 20
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--calls", str(calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        if p.returncode != 0:
            return {"error": "rocprofv3 run ended with %d" % p.returncode, "tail": p.stdout.decode(errors="replace")[-400:]}
        seq = trace_times(d)
        if isinstance(seq, dict):
            return seq
        res, pos = {}, 0
        for name, sizes, both in LAYOUTS:
            want = ([("lwf_loss_kernel",)] * calls if both else []) + [("lwf_wide_rows_kernel", "lwf_wide_sum_kernel")] * calls
            flat = [k for grp in want for k in grp]
            part = seq[pos:pos + len(flat)]
            pos += len(flat)
            if [k for k, _ in part] != flat:
                return {"error": "the trace does not follow the launch order at layout " + name}
            by = {}
            for k, ns in part:
                by.setdefault(k, []).append(ns / 1000.0)
            res[name] = {k + "_avg_us": sum(v) / len(v) for k, v in by.items()}
        return res


def child(a):
    """What the profiled run does: per layout --calls narrow calls (where the kernel takes it), then --calls wide calls; kernel
    durations in the trace do not include code-object loading, so there is no warm-up to separate."""
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    for name, sizes, both in LAYOUTS:
        narrow, wide, keep = make_calls(L, torch, sizes)
        if both:
            for _ in range(a.calls):
                narrow()
        for _ in range(a.calls):
            wide()
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lwf_loss_bench needs the GPU: a CPU run measures nothing")
    from clsurvey_amd import _lib
    L = _lib.lib()
    res = {"N": N, "T": T, "rounds": a.rounds, "calls_per_round": a.calls, "layouts": {}}
    fns = [(name, both) + make_calls(L, torch, sizes) for name, sizes, both in LAYOUTS]
    for _ in range(a.warmup):
        for name, both, narrow, wide, keep in fns:
            if both:
                timed(torch, narrow, a.calls)
            timed(torch, wide, a.calls)
    times = {name: {"narrow": [], "wide": []} for name, *_ in fns}
    for _ in range(a.rounds):
        for name, both, narrow, wide, keep in fns:
            if both:
                times[name]["narrow"].append(timed(torch, narrow, a.calls))
            times[name]["wide"].append(timed(torch, wide, a.calls))
    for name, both, *_ in fns:
        entry = {"wide": summary(times[name]["wide"])}
        if both:
            entry["narrow"] = summary(times[name]["narrow"])
            entry["wide_over_narrow"] = entry["wide"]["median_us"] / entry["narrow"]["median_us"]
            spread = max(entry["wide"]["spread"], entry["narrow"]["spread"])
            entry["wide_slower_beyond_spread"] = entry["wide"]["median_us"] > entry["narrow"]["median_us"] * (1.0 + spread)
        res["layouts"][name] = entry
    if a.profile:
        res["kernel_trace_avg_us"] = profile_child(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
