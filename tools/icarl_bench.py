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
python tools/icarl_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/icarl_bench.json]
  --herd_wide: herding ALONE over synthetic features (no net): 20 classes x 400 rows, K = 51 and K = 400, four variants that
      alternate inside every round:
        narrow_4096    clhip_icarl_herd at F = 4096 (mu, S, r in LDS)
        wide_4096      clhip_icarl_herd_wide forced at the same features: what mu and S in device memory cost (never chosen there)
        wide_8192      clhip_icarl_herd_wide at wide_VGG9's width
        wide_16384     ... at deep_VGG22's
python tools/icarl_bench.py --herd_wide [--rounds 7] [--out profiles/icarl_wide_bench.json]"""
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


def herd_wide(a):
    from clsurvey_amd import ops
    from clsurvey_amd.methods.icarl import mean_weights
    gen = torch.Generator(device="cuda").manual_seed(38)
    n = 8000
    z = torch.randn((n, 3), device="cuda", generator=gen)

    def feats(F):                                  # the tests' features: a ReLU of a rank-3 pattern plus noise
        return torch.relu(z @ torch.randn((3, F), device="cuda", generator=gen) + 0.05 * torch.randn((n, F), device="cuda", generator=gen))
    f = {F: feats(F) for F in (4096, 8192, 16384)}
    ranges = [(400 * c, 400 * (c + 1)) for c in range(20)]
    wts = torch.from_numpy(np.concatenate([mean_weights(400, 132)] * 20)).cuda()
    res = {"classes": 20, "rows_per_class": 400, "features": "relu(rank-3 pattern + 0.05 noise)"}
    for K in (51, 400):
        ks = [K] * 20
        fns = {"narrow_4096": lambda: ops.icarl_herd(f[4096], wts, ranges, ks, flat=True, wide=False),
               "wide_4096": lambda: ops.icarl_herd(f[4096], wts, ranges, ks, flat=True, wide=True),
               "wide_8192": lambda: ops.icarl_herd(f[8192], wts, ranges, ks, flat=True),
               "wide_16384": lambda: ops.icarl_herd(f[16384], wts, ranges, ks, flat=True)}
        t = timed_together(fns, 1, 2, a.rounds)        # millisecond-scale calls: one call per window
        out = {name: summary(v) for name, v in t.items()}
        out["rankings_equal_at_4096"] = bool(torch.equal(fns["narrow_4096"]()[0], fns["wide_4096"]()[0]))
        out["wide_over_narrow_at_4096"] = out["wide_4096"]["median_us"] / out["narrow_4096"]["median_us"]
        res["K%d" % K] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--herd_wide", action="store_true", help="time herding alone at F = 4096 (both entries), 8192 and 16384")
    a = ap.parse_args()
    if a.herd_wide:
        res = herd_wide(a)
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
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
