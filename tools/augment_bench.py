"""One augmented batch of 200 out of 10 tasks, timed with HIP events (medians and spread over repeated rounds, the variants
alternating inside every round), at 3 x 72^2 -> 64^2 and 3 x 256^2 -> 224^2:
  kernel          clhip_gather_tasks_crop_flip out of the per-task frames: one launch
  index_select    x.index_select(0, idx) + y.index_select(0, idx) on a merged tensor of the OUTPUT's size: what the un-augmented
                  loader pays, and the floor for the bytes written
  torch_ops       the same crop + flip by torch ops: index_select of the full frames of a merged copy (a B x C x Hs x Ws
                  intermediate), then one batched gather (advanced indexing with per-sample line and column tables)
  torch_direct    that batched gather straight out of the merged copy, no intermediate (still needs the merged copy)
bytes = what a variant has to move at the least: output read + written (2 x B C th tw x 4) for kernel / index_select /
torch_direct, plus the intermediate written and read again (2 x B C Hs Ws x 4) for torch_ops; share_of_8TBps = bytes / time / 8e12
(the HBM figure of bench.py's roofline).
python tools/augment_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/augment_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_together(fns, iters, warmup, rounds):
    """{name: [microseconds per call]}: the variants ALTERNATE inside every round (one window of `iters` calls each between
    two HIP events), so that clock and neighbour drift hit them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1000.0 / iters)
    return out


def summary(v, nbytes):
    med = statistics.median(v)
    return {"median_us": med, "min_us": min(v), "max_us": max(v), "rounds": len(v), "bytes": nbytes,
            "share_of_8TBps": nbytes / (med * 1e-6) / 8e12}


def case(C, Hs, th, n_per_task, a, T=10, B=200):
    from clsurvey_amd import ops
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    Ws, tw = Hs, th
    dev = "cuda"
    xs = [torch.randn((n_per_task, C, Hs, Ws), device=dev) for _ in range(T)]
    ys = [torch.randint(0, 20, (n_per_task,), device=dev) for _ in range(T)]
    cum = [n_per_task * (j + 1) for j in range(T)]
    shifts = [20 * j for j in range(T)]
    table = ops.task_table(xs, ys, cum, shifts, dev)
    merged = torch.cat(xs)                                             # torch_ops / torch_direct need the merged copy
    merged_y = torch.cat([y + s for y, s in zip(ys, shifts)])
    small = torch.randn((T * n_per_task, C, th, tw), device=dev)      # index_select: a dataset of the output's size
    g = torch.Generator().manual_seed(1)
    idx = torch.randperm(T * n_per_task, generator=g)[:B].to(dev)
    params = draw_crop_flip(B, RandomCropFlip((th, tw)), (Hs, Ws), g).to(dev)
    geometry = (C, Hs, Ws, th, tw)
    ar_b = torch.arange(B, device=dev)[:, None, None, None]
    ar_c = torch.arange(C, device=dev)[None, :, None, None]
    ar_h, ar_w = torch.arange(th, device=dev), torch.arange(tw, device=dev)

    def tables():
        top, left, flip = params[:, 0].long(), params[:, 1].long(), params[:, 2:3] == 1
        lines = (top[:, None] + ar_h)[:, None, :, None]
        cols = (left[:, None] + torch.where(flip, tw - 1 - ar_w, ar_w))[:, None, None, :]
        return lines, cols

    def kernel():
        return ops.gather_tasks_crop_flip(table, geometry, idx, params)

    def index_select():
        return small.index_select(0, idx), merged_y.index_select(0, idx)

    def torch_ops():
        lines, cols = tables()
        return merged.index_select(0, idx)[ar_b, ar_c, lines, cols], merged_y.index_select(0, idx)

    def torch_direct():
        lines, cols = tables()
        return merged[idx[:, None, None, None], ar_c, lines, cols], merged_y.index_select(0, idx)

    want = kernel()
    for fn in (torch_ops, torch_direct):
        got = fn()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), fn.__name__
    out_bytes, full_bytes = 2 * B * C * th * tw * 4, 2 * B * C * Hs * Ws * 4
    t = timed_together({"kernel": kernel, "index_select": index_select, "torch_ops": torch_ops, "torch_direct": torch_direct},
                       a.iters, a.warmup, a.rounds)
    res = {"geometry": list(geometry), "tasks": T, "batch": B, "frames_per_task": n_per_task,
           "kernel": summary(t["kernel"], out_bytes), "index_select": summary(t["index_select"], out_bytes),
           "torch_ops": summary(t["torch_ops"], out_bytes + full_bytes), "torch_direct": summary(t["torch_direct"], out_bytes)}
    res["kernel_over_index_select"] = res["kernel"]["median_us"] / res["index_select"]["median_us"]
    res["torch_ops_over_kernel"] = res["torch_ops"]["median_us"] / res["kernel"]["median_us"]
    res["torch_direct_over_kernel"] = res["torch_direct"]["median_us"] / res["kernel"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"72_to_64": case(3, 72, 64, 2000, a), "256_to_224": case(3, 256, 224, 400, a)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
