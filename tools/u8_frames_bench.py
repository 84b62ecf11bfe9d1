"""One batch of 200 out of 10 tasks x 2000 frames held as uint8 against the same batch out of their decoded fp32 twins, timed
with HIP events (medians and spread over repeated rounds, the two entries of a pair alternating inside every round), at
3 x 72^2 -> 64^2 and 3 x 256^2 -> 224^2, one process:
  plain      clhip_gather_tasks_u8                    against clhip_gather_tasks                    (whole frames, no crop)
  crop_flip  clhip_gather_tasks_crop_flip_u8          against clhip_gather_tasks_crop_flip
  resized    clhip_gather_tasks_resized_crop_flip_u8  against clhip_gather_tasks_resized_crop_flip  (windows of the default spec)
The two batches of a pair are compared bitwise before anything is timed.  source_bytes = what a batch has to read at the least,
C Hs Ws B x {1, 4} (the whole frame for plain, and an upper bound for the windows of the other two); resident_bytes = what the
sequence takes in HBM in either form.
python tools/u8_frames_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--frames 2000] [--out profiles/u8_frames_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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


def summary(v, source_bytes):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v), "source_bytes": source_bytes}


def case(C, Hs, th, n_per_task, a, T=10, B=200):
    from clsurvey_amd import ops
    from clsurvey_amd.data import (ByteTaskDataset, RandomCropFlip, RandomResizedCropFlip, draw_crop_flip, draw_resized_crop_flip)
    Ws, tw = Hs, th
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1)
    ys = [torch.randint(0, 20, (n_per_task,), device=dev, generator=gen) for _ in range(T)]
    byte = [ByteTaskDataset(torch.randint(0, 256, (n_per_task, C, Hs, Ws), device=dev, dtype=torch.uint8, generator=gen), y, [],
                            MEAN[:C], STD[:C]) for y in ys]
    xb = [d.x for d in byte]
    xf = [d.decoded().x for d in byte]
    cum = [n_per_task * (j + 1) for j in range(T)]
    shifts = [20 * j for j in range(T)]
    tb, tf = ops.task_table(xb, ys, cum, shifts, dev), ops.task_table(xf, ys, cum, shifts, dev)
    lut = byte[0].lut().to(dev)
    g = torch.Generator().manual_seed(1)
    idx = torch.randperm(T * n_per_task, generator=g)[:B].to(dev)
    p3 = draw_crop_flip(B, RandomCropFlip((th, tw)), (Hs, Ws), g).to(dev)
    p5 = draw_resized_crop_flip(B, RandomResizedCropFlip((th, tw)), (Hs, Ws), g).to(dev)
    geometry = (C, Hs, Ws, th, tw)
    x_full = torch.empty((B, C * Hs * Ws), device=dev)
    x_crop = torch.empty((B, C, th, tw), device=dev)
    y_out = torch.empty((B,), dtype=torch.int64, device=dev)
    pairs = {
        "plain": (lambda: ops.gather_tasks_u8(tb, C, Hs * Ws, lut, idx, x_out=x_full, labels_out=y_out),
                  lambda: ops.gather_tasks(tf, C * Hs * Ws, idx, x_out=x_full, labels_out=y_out)),
        "crop_flip": (lambda: ops.gather_tasks_crop_flip_u8(tb, geometry, lut, idx, p3, x_out=x_crop, labels_out=y_out),
                      lambda: ops.gather_tasks_crop_flip(tf, geometry, idx, p3, x_out=x_crop, labels_out=y_out)),
        "resized": (lambda: ops.gather_tasks_resized_crop_flip_u8(tb, geometry, lut, idx, p5, x_out=x_crop, labels_out=y_out),
                    lambda: ops.gather_tasks_resized_crop_flip(tf, geometry, idx, p5, x_out=x_crop, labels_out=y_out)),
    }
    src = C * Hs * Ws * B
    res = {"geometry": list(geometry), "tasks": T, "batch": B, "frames_per_task": n_per_task,
           "resident_bytes": {"u8": sum(x.numel() for x in xb), "fp32": sum(4 * x.numel() for x in xf)}}
    for name, (u8, fp32) in pairs.items():
        got = [v.clone() for v in u8()]
        want = [v.clone() for v in fp32()]
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), name
        t = timed_together({"u8": u8, "fp32": fp32}, a.iters, a.warmup, a.rounds)
        res[name] = {"u8": summary(t["u8"], src), "fp32": summary(t["fp32"], 4 * src)}
        res[name]["u8_over_fp32"] = res[name]["u8"]["median_us"] / res[name]["fp32"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2000, help="frames per task")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name, (C, Hs, th) in (("72_to_64", (3, 72, 64)), ("256_to_224", (3, 256, 224))):
        res[name] = case(C, Hs, th, a.frames, a)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
