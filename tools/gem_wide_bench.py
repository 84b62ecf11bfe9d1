"""GEM's solver on a 64-task sequence against the memory passes of the same observe, on small_VGG9_cl_128_128 at 64x64 (64
tasks of 2 classes, n_memories = batch = 10), HIP-event timed, one process, median of --iters repeats after --warmup:
  (a) chain_wide    GemNet.project_on_device with 63 memory rows: clhip_gem_gram_wide -> clhip_gem_qp_wide ->
                    clhip_gem_project_dev_wide, for the "margin-boundary" and "all-violated" pinned problems of
                    tests/test_gpu_gem_kernels.py::chain_problem at the model's parameter count; and its three launches alone
  (b) memory_passes the 63 past-task passes (engine.loss_step + clhip_axpy) that the same observe runs before the solver
  (c) chain_narrow  the same chain with 15 memory rows (csrc/gem.hip), for scale
The Gram pass is reported as a fraction of the 8 TB/s HBM3E spec for m * n * 4 bytes.
python tools/gem_wide_bench.py [--iters 20] [--warmup 3] [--out profiles/gem_wide.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12
N_TASKS, NC, N_MEM = 64, 2, 10


def chain_problem(kind, t, n):
    """The recipe of tests/test_gpu_gem_kernels.py::chain_problem (rows on the grid k / 16: the Gram matrix is exact in f64)."""
    rs = np.random.RandomState(100 * t + len(kind))
    M = rs.randint(-8, 9, size=(t, n)).astype(np.float32) / 8
    g = rs.randint(-8, 9, size=n).astype(np.float32) / 8
    margin = 0.0
    if kind == "all-violated":
        c = rs.randint(-8, 9, size=n).astype(np.float32) / 8
        M = M / 2 + c
        g = -c
    else:
        margin = 0.5
        g = g / 4 - 2 * M[0] - M[t - 1]
    return M, g, margin


def medians(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from clsurvey_amd import _lib, models
    from clsurvey_amd.methods.gem import GemNet, _stream, compute_offsets, extend_head
    L = _lib.lib()
    torch.manual_seed(5)
    net = extend_head(models.parse_model_name("small_VGG9_cl_128_128", (64, 64), NC), NC * N_TASKS)
    gem = GemNet(net, NC * N_TASKS, N_TASKS, [NC] * N_TASKS, N_MEM, 1e-3, 0.0, 0.5, batch_size=N_MEM, in_shape=(3, 64, 64), device="cuda")
    n = gem.A.numel
    res = {"model": "small_VGG9_cl_128_128", "hw": 64, "n_params": n, "n_tasks": N_TASKS, "n_memories": N_MEM, "iters": a.iters}

    def load(kind, t):
        M, g, margin = chain_problem(kind, t, n)
        gem.G[:t].copy_(torch.from_numpy(M))
        gem.G[t].copy_(torch.from_numpy(g))
        gem.margin = margin

    for kind in ("margin-boundary", "all-violated"):
        for t, name in ((63, "chain_wide"), (15, "chain_narrow")):
            load(kind, t)
            rows = list(range(t))
            res["%s_us[%s]" % (name, kind)] = medians(lambda: gem.project_on_device(rows, t), a.iters, a.warmup)
            gem.check_qp_status()
            res["violated[%s][t=%d]" % (kind, t)] = int(gem._info[0].item())
        # the three launches of the wide chain alone (the buffers hold the t = 63 problem's Gram matrix and v again afterwards)
        load(kind, 63)
        m = 64
        idx, idx_mem = (C.c_int * m)(*range(m)), (C.c_int * (m - 1))(*range(m - 1))
        G, ld = gem.G.data_ptr(), gem.G.shape[1]

        def gram():
            L.clhip_gem_gram_wide(G, ld, idx, m, n, gem._gram.data_ptr(), gem._gram_ws.data_ptr(), gem._gram_ws.numel(), _stream())

        def qp():
            L.clhip_gem_qp_wide(gem._gram.data_ptr(), m, float(gem.margin), 1e-3, gem._v.data_ptr(), gem._info.data_ptr(),
                                gem._qp_ws.data_ptr(), gem._qp_ws.numel(), _stream())

        def project():
            L.clhip_gem_project_dev_wide(G, ld, idx_mem, gem._v.data_ptr(), gem._info.data_ptr(), m - 1, gem.G[m - 1].data_ptr(),
                                         gem.A.grad.data_ptr(), n, _stream())
        for name, fn in (("gram_wide", gram), ("qp_wide", qp), ("project_dev_wide", project)):
            res["%s_us[%s]" % (name, kind)] = medians(fn, a.iters, a.warmup)
        us = res["gram_wide_us[%s]" % kind]
        res["gram_wide_TBps[%s]" % kind] = m * n * 4 / (us * 1e-6) / 1e12
        res["gram_wide_of_hbm_spec[%s]" % kind] = m * n * 4 / (us * 1e-6) / HBM_SPEC

    # the Gram pass alone over the row count (1, 3, 6, 10 panel pairs): time, and the rate of m * n * 4 bytes against the HBM spec
    for mm in (16, 32, 48, 64):
        idx_m = (C.c_int * mm)(*range(mm))
        us = medians(lambda: L.clhip_gem_gram_wide(G, ld, idx_m, mm, n, gem._gram.data_ptr(), gem._gram_ws.data_ptr(),
                                                   gem._gram_ws.numel(), _stream()), a.iters, a.warmup)
        res["gram_wide_us[m=%d]" % mm] = us
        res["gram_wide_of_hbm_spec[m=%d]" % mm] = mm * n * 4 / (us * 1e-6) / HBM_SPEC
    idx16 = (C.c_int * 16)(*range(16))
    us = medians(lambda: L.clhip_gem_gram(G, ld, idx16, 16, n, gem._gram.data_ptr(), gem._gram_ws.data_ptr(), gem._gram_ws.numel(),
                                          _stream()), a.iters, a.warmup)
    res["gram_narrow_us[m=16]"] = us

    # (b) the 63 memory passes of an observe of the 64th task
    gem.memory_x.normal_()
    gem.memory_labels.copy_(torch.arange(N_TASKS, device="cuda").view(-1, 1) * NC + torch.randint(0, NC, (N_TASKS, N_MEM), device="cuda"))
    gem._dropout(True)

    def passes():
        for past in range(N_TASKS - 1):
            sl = compute_offsets(past, gem.cum_nc_per_task)
            first = True
            for xb, yb in gem._memory_loader(past):
                gem.engine.loss_step(xb.contiguous(), yb.contiguous(), "ce_mean", True, class_slice=sl)
                gem._axpy(gem.G[past], assign=first)
                first = False
    res["memory_passes_us"] = medians(passes, a.iters, a.warmup)
    for kind in ("margin-boundary", "all-violated"):
        res["chain_wide_over_memory_passes[%s]" % kind] = res["chain_wide_us[%s]" % kind] / res["memory_passes_us"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
