"""One rehearsal-baseline step on small_VGG9_cl_128_128 at 64x64 and the task-10 shape (200 current images + 68 exemplars
of 9 past tasks, N = 268), timed three ways with HIP events:
  fused      RehearsalNet.observe_FT: clhip_rehearsal_assemble + clhip_net_loss_step_loss_segments + SGD
  segmented  the same step, one loss_step per exemplar chunk + current batch, clhip_axpy accumulation (the BatchNorm path)
  plain      loss_step + SGD over 268 images (no plan, no assembly): the floor the fused step is held against
python tools/rehearsal_step_bench.py [--iters 50] [--warmup 10] [--out profiles/rehearsal_step.json]"""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wrapper(segmented):
    from clsurvey_amd import models
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    torch.manual_seed(5)
    net = replace_head(models.parse_model_name("small_VGG9_cl_128_128", (64, 64), 20), 200)
    w = RehearsalNet(net, 200, 10, [20] * 10, 450, 1e-3, 0.0, False, 268, (3, 64, 64), "cuda")
    w.init_setup(lr=1e-3, weight_decay=0.0, n_append=68, chunk_size=132)
    w.store_x[:9 * 450].normal_()
    w.store_y[:9 * 450].random_(0, 20)
    w.observed_tasks, w.old_task, w.filled = list(range(9)), 9, [450] * 10
    w.observed_tasks.append(9)
    w.force_segmented = segmented
    return w


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    random.seed(0)
    x = torch.randn((200, 3, 64, 64), device="cuda")
    y = torch.randint(0, 20, (200,), device="cuda")
    res = {"model": "small_VGG9_cl_128_128", "hw": 64, "current": 200, "exemplars": 68, "past_tasks": 9, "iters": a.iters}
    for name, seg in (("fused_us", False), ("segmented_us", True)):
        w = wrapper(seg)
        res[name] = timed(lambda: w.observe_FT(x, 9, y), a.iters, a.warmup)
    w = wrapper(False)
    xp = torch.randn((268, 3, 64, 64), device="cuda")
    yp = torch.randint(0, 20, (268,), device="cuda")
    w._dropout(True)

    def plain():
        w.engine.loss_step(xp, yp, "ce_mean", True, class_slice=(180, 200))
        w.opt.step()
    res["plain_us"] = timed(plain, a.iters, a.warmup)
    res["fused_over_plain"] = res["fused_us"] / res["plain_us"]
    res["fused_over_segmented"] = res["fused_us"] / res["segmented_us"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
