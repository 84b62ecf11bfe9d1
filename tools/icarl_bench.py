"""iCaRL on small_VGG9_cl_128_128 at 64x64, timed with HIP events (medians and spread over repeated rounds):
  (a) herding of one Tiny-ImageNet-sized task: 20 classes x 400 images, features of the train split computed once, K from
      mem_per_task = 1024 at task 1 (K/m = 512 -> every class ranks all 400 images) and at task 10 (K/m = 51):
        herd_us        clhip_icarl_herd, one launch for the 20 classes
        torch_us       the same ranking by torch ops on the same device over the same features (one cost vector per pick)
        features_us    the feature pass both share (8000 images through the plan)
  (b) one update_representation step at task 10 (200 current images + 68 exemplars of 9 past tasks, N = 268):
        fused_us       IcarlNet.observe: assemble + clhip_net_loss_step_loss_segments + SGD
        segmented_us   the same step, one pass per chunk (the BatchNorm path)
        plain_us       loss_step + SGD over 268 images: the floor
python tools/icarl_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/icarl_bench.json]"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
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


def timed(fn, iters, warmup, rounds):
    return timed_together({"x": fn}, iters, warmup, rounds)["x"]


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v)}


def wrapper(segmented):
    from clsurvey_amd import models
    from clsurvey_amd.methods.icarl import IcarlNet
    torch.manual_seed(5)
    net = models.parse_model_name("small_VGG9_cl_128_128", (64, 64), 20)
    w = IcarlNet(net, 200, 10, [20] * 10, 1024, 1e-3, 0.0, 10.0, 268, (3, 64, 64), "cuda")
    w.init_setup(lr=1e-3, weight_decay=0.0, memory_strength=10.0, n_append=68, chunk_size=132, total_batch_size=200)
    w.exemplar_count = 10240 // 180
    w.class_len = [w.exemplar_count] * 180
    w.store_x[:180 * w.exemplar_count].normal_()
    w.store_t[:180 * w.exemplar_count].normal_()
    w.observed_tasks, w.old_task = list(range(10)), 9
    w.force_segmented = segmented
    return w


def torch_herd(feats, w, ranges, ks):
    out = []
    for (lo, hi), K in zip(ranges, ks):
        f = feats[lo:hi]
        mu = (f * w[lo:hi, None]).sum(0)
        prev = torch.zeros_like(mu)
        taken = torch.zeros(hi - lo, dtype=torch.bool, device=f.device)
        rank = torch.empty(K, dtype=torch.int64, device=f.device)
        for k in range(K):
            cost = (mu - (f + prev) / (k + 1)).norm(2, 1)
            cost[taken] = float("inf")
            win = cost.argmin()
            rank[k] = win
            taken[win] = True
            prev = prev + f[win]
        out.append(rank)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from clsurvey_amd.methods.icarl import mean_weights
    random.seed(0)
    np.random.seed(0)
    res = {"model": "small_VGG9_cl_128_128", "hw": 64}
    w = wrapper(False)
    xs = torch.randn((8000, 3, 64, 64), device="cuda")
    w.net.train(False)
    w._dropout(1)
    res["features"] = summary(timed(lambda: w.features(xs), 1, 1, a.rounds))
    feats = w.features(xs)
    ranges = [(400 * c, 400 * (c + 1)) for c in range(20)]
    wts = torch.from_numpy(np.concatenate([mean_weights(400, 132)] * 20)).cuda()
    for tag, K in (("task1_K400", 400), ("task10_K51", 51)):
        ks = [K] * 20
        both = timed_together({"herd": lambda: w.herd(feats, ranges, wts, ks), "torch": lambda: torch_herd(feats, wts, ranges, ks)},
                              1, 2, a.rounds)                 # millisecond-scale calls: one call per window
        herd, ref = both["herd"], both["torch"]
        got = w.herd(feats, ranges, wts, ks)[0].view(20, K).long()
        same = sum(int(torch.equal(g, r)) for g, r in zip(got, torch_herd(feats, wts, ranges, ks)))
        res["herd_" + tag] = {"herd": summary(herd), "torch": summary(ref), "classes_with_equal_ranking": same,
                              "torch_over_herd": statistics.median(ref) / statistics.median(herd)}
    x = torch.randn((200, 3, 64, 64), device="cuda")
    y = torch.randint(0, 20, (200,), device="cuda")
    wf, wseg = wrapper(False), wrapper(True)
    wp = wrapper(False)
    xp = torch.randn((268, 3, 64, 64), device="cuda")
    yp = torch.randint(0, 20, (268,), device="cuda")
    wp.net.train(True)
    wp._dropout(268)

    def plain():
        wp.engine.loss_step(xp, yp, "ce_mean", True, class_slice=(180, 200))
        wp.opt.step()
    steps = timed_together({"fused": lambda: wf.observe(x, 9, y), "segmented": lambda: wseg.observe(x, 9, y), "plain": plain},
                           a.iters, a.warmup, a.rounds)
    for name, v in steps.items():
        res[name] = summary(v)
    res["fused_over_plain"] = res["fused"]["median_us"] / res["plain"]["median_us"]
    res["fused_over_segmented"] = res["fused"]["median_us"] / res["segmented"]["median_us"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
