"""Milliseconds per PathNet training step next to the plain finetuning step of the same build, on the same device in the same
process: small_VGG9_cl_128_128 at 3 x 64 x 64, batch 200.
  pathnet    PathEngine.step with N = 3, M = 20 (the method row's defaults): pack, the plan over the packed net (every width
             padded to 32 channels) with CE, fold, clip + SGD — the plan's own launches plus three
  finetune   NetEngine.loss_step over the full-width net + clhip_reg_sgd_step with lambda = 0 (what the SGD baseline runs)
Host clock around a device synchronise, `--iters` steps per window; the two variants alternate inside every round and the
medians and the spread over rounds are reported.  The PathNet step trains a net of 3/20 of the width: the figures say what the
three extra launches and the padding cost, not which method is faster.
python tools/pathnet_step_time.py [--rounds 7] [--iters 50] [--warmup 10] [--only pathnet|finetune] [--out profiles/pathnet_step_time.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--only", default="", help="time one variant only (for a kernel trace of it): pathnet | finetune")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pathnet_step_time: needs the GPU (no CPU timing is reported)")
    from clsurvey_amd import models, net, ops
    from clsurvey_amd.methods import pathnet as PN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shape, ncls, N, M = (3, 64, 64), 20, 3, 20
    x = torch.randn((a.batch,) + shape, device=dev)
    y = torch.randint(0, ncls, (a.batch,), device=dev)

    pnet = PN.PathNet(models.parse_model_name("small_VGG9_cl_128_128", shape[1:], ncls), shape, [(0, ncls)], [N, M])
    eng = PN.PathEngine(pnet, a.batch, shape, dev)
    pnet.train()
    eng.set_path(np.stack([np.random.RandomState(l).permutation(M)[:N] for l in range(pnet.L)]), 0)
    opt = PN.PathSGD(eng, 0.01, 0.9, 5e-4)

    plain = models.parse_model_name("small_VGG9_cl_128_128", shape[1:], ncls)
    plain.train()
    peng = net.NetEngine(plain, a.batch, shape, dev)
    A = peng.arena
    zeros, buf = A.buffer("omega"), A.buffer("buf")
    first = [True]

    def pathnet_step():
        eng.step(x, y, opt, 1000.0)

    def finetune_step():
        peng.loss_step(x, y, "ce_mean", True)
        ops.reg_sgd_step(A.theta, A.grad, zeros, zeros, buf, 0.0, 0.01, 0.9, 5e-4, first[0])
        first[0] = False

    variants = {"pathnet": pathnet_step, "finetune": finetune_step}
    if a.only:
        variants = {a.only: variants[a.only]}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for r in range(a.rounds):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for k in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                variants[k]()
            torch.cuda.synchronize()
            ms[k].append(1000 * (time.perf_counter() - t0) / a.iters)
    out = {"model": "small_VGG9_cl_128_128", "input": list(shape), "batch": a.batch, "N": N, "M": M, "granule": PN.GRANULE,
           "packed_widths": [g["Kp"] for g in eng._geo], "iters": a.iters, "rounds": a.rounds,
           "extra_launches_per_step": 3,
           "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
