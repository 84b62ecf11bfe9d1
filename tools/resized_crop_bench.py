"""One RandomResizedCrop + flip batch of 200 out of 10 tasks, timed with HIP events (medians and spread over repeated rounds, the
variants alternating inside every round), at 3 x 64^2 -> 56^2 (the cropped Tiny-ImageNet variant) and 3 x 256^2 -> 224^2, windows
drawn from the default spec (scale 0.08 - 1, ratio 3/4 - 4/3):
  kernel          clhip_gather_tasks_resized_crop_flip out of the per-task frames: one launch
  crop_flip       clhip_gather_tasks_crop_flip at the same output geometry: the floor (the same bytes written, no filtering)
  torch_ops       the same batch by torch ops on the same device: index_select of the full frames of a merged copy (a
                  B x C x Hs x Ws intermediate), then per sample the window slice, F.interpolate(mode="bilinear",
                  antialias=True), the flip, written into the output batch
bytes = what a variant has to move at the least: kernel the windows read + the output written, crop_flip the output read +
written, torch_ops the intermediate written and read again + the output written; share_of_8TBps = bytes / time / 8e12 (the HBM
figure of bench.py's roofline).
python tools/resized_crop_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/resized_crop_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_together(fns, iters, warmup, rounds):
    """{name: [microseconds per call]}: the variants ALTERNATE inside every round (one window of `iters` calls each between
    two HIP events), so that clock and neighbour drift hit them alike.  fns: {name: (fn, iters)}."""
    for fn, _ in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, (fn, n) in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1000.0 / n)
    return out


def summary(v, nbytes):
    med = statistics.median(v)
    return {"median_us": med, "min_us": min(v), "max_us": max(v), "rounds": len(v), "bytes": nbytes,
            "share_of_8TBps": nbytes / (med * 1e-6) / 8e12}


def case(C, Hs, th, n_per_task, a, T=10, B=200):
    from clsurvey_amd import ops
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip, draw_crop_flip, draw_resized_crop_flip
    Ws, tw = Hs, th
    dev = "cuda"
    xs = [torch.randn((n_per_task, C, Hs, Ws), device=dev) for _ in range(T)]
    ys = [torch.randint(0, 20, (n_per_task,), device=dev) for _ in range(T)]
    cum = [n_per_task * (j + 1) for j in range(T)]
    shifts = [20 * j for j in range(T)]
    table = ops.task_table(xs, ys, cum, shifts, dev)
    merged = torch.cat(xs)                                             # torch_ops needs the merged copy
    merged_y = torch.cat([y + s for y, s in zip(ys, shifts)])
    g = torch.Generator().manual_seed(1)
    idx = torch.randperm(T * n_per_task, generator=g)[:B].to(dev)
    host = draw_resized_crop_flip(B, RandomResizedCropFlip((th, tw)), (Hs, Ws), g)
    params = host.to(dev)
    crop_params = draw_crop_flip(B, RandomCropFlip((th, tw)), (Hs, Ws), g).to(dev)
    rows = host.tolist()
    geometry = (C, Hs, Ws, th, tw)

    def kernel():
        return ops.gather_tasks_resized_crop_flip(table, geometry, idx, params)

    def crop_flip():
        return ops.gather_tasks_crop_flip(table, geometry, idx, crop_params)

    def torch_ops():
        full = merged.index_select(0, idx)
        out = torch.empty((B, C, th, tw), device=dev)
        for b, (top, left, h, w, flip) in enumerate(rows):
            v = F.interpolate(full[b:b + 1, :, top:top + h, left:left + w], size=(th, tw), mode="bilinear", align_corners=False,
                              antialias=True)
            out[b] = v[0].flip(-1) if flip else v[0]
        return out, merged_y.index_select(0, idx)

    want, got = kernel(), torch_ops()
    parity = float((want[0] - got[0]).abs().max())                     # two fp32 evaluations of one formula
    assert torch.equal(want[1], got[1]) and parity < 1e-3, parity
    out_bytes, full_bytes = B * C * th * tw * 4, B * C * Hs * Ws * 4
    window_bytes = int((host[:, 2].long() * host[:, 3].long()).sum()) * C * 4
    t = timed_together({"kernel": (kernel, a.iters), "crop_flip": (crop_flip, a.iters), "torch_ops": (torch_ops, max(1, a.iters // 10))},
                       a.iters, a.warmup, a.rounds)
    res = {"geometry": list(geometry), "tasks": T, "batch": B, "frames_per_task": n_per_task,
           "mean_window_side": float((host[:, 2].double() * host[:, 3].double()).mean().sqrt()),
           "max_abs_difference_kernel_vs_torch_ops": parity,
           "kernel": summary(t["kernel"], window_bytes + out_bytes), "crop_flip": summary(t["crop_flip"], 2 * out_bytes),
           "torch_ops": summary(t["torch_ops"], 2 * full_bytes + out_bytes)}
    res["kernel_over_crop_flip"] = res["kernel"]["median_us"] / res["crop_flip"]["median_us"]
    res["torch_ops_over_kernel"] = res["torch_ops"]["median_us"] / res["kernel"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"64_to_56": case(3, 64, 56, 2000, a), "256_to_224": case(3, 256, 224, 400, a)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
