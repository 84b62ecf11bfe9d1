"""The batch assembly of a task-10 R-PM step on RESIZED tasks (the step shape of tools/exemplar_augment_bench.py: 200 current rows,
the exemplar rows exemplar_split gives for 450 memories per task and 8000 training images, the ring update of 200 rows), timed
with HIP events (medians and spread over repeated rounds, the variants alternating inside every round), at 3 x 72^2 -> 64^2 and
3 x 256^2 -> 224^2, windows drawn by the default RandomResizedCropFlip:
  fused           clhip_rehearsal_assemble_resized_crop_flip on a store of frames: current rows, ring update by sample number,
                  exemplars resampled; one launch (every block carries the plan's dynamic LDS)
  two_launch      what could be composed without that kernel: clhip_rehearsal_assemble_crop_flip with E = 0 for the copy and ring
                  rows plus clhip_gather_tasks_resized_crop_flip over the store for the exemplar rows
  crop_fused      clhip_rehearsal_assemble_crop_flip on the same store (exemplars cropped, not resampled): the price of resampling
bytes = read + written of every row a variant moves, with a resized window counted at its own size; share_of_8TBps = bytes / time /
8e12 (the HBM figure of bench.py's roofline).
Then the WHOLE step of RehearsalNet.observe_FT at 64^2 (host plan and draws, upload, assembly, one fused engine pass of
small_VGG9_cl_128_128, SGD) with a RandomCropFlip and with a RandomResizedCropFlip spec, host clock around a device synchronise.
python tools/exemplar_resized_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/exemplar_resized_bench.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.augment_bench import summary, timed_together  # noqa: E402
from tools.exemplar_augment_bench import N_MEM, N_TASKS, step_shape  # noqa: E402


def kernel_case(C, Hs, th, a):
    from clsurvey_amd import ops
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip, draw_crop_flip, draw_resized_crop_flip
    B, E, _ = step_shape()
    Ws, tw = Hs, th
    dev = "cuda"
    rows = N_TASKS * N_MEM
    g = torch.Generator().manual_seed(1)
    frames = torch.randn((2000 if Hs < 100 else 400, C, Hs, Ws), device=dev)          # the current task's loader frames
    src_idx = torch.randperm(frames.shape[0], generator=g)[:B].to(dev)
    x = torch.randn((B, C, th, tw), device=dev)
    y = torch.randint(0, 20, (B,), device=dev)
    store = torch.randn((rows, C, Hs, Ws), device=dev)
    store_y = torch.randint(0, 20, (rows,), device=dev)
    gather = torch.randperm((N_TASKS - 1) * N_MEM, generator=g)[:E].to(torch.int32).to(dev)      # rows of the nine past tasks
    windows = draw_resized_crop_flip(E, RandomResizedCropFlip((th, tw)), (Hs, Ws), g)
    params5 = windows.to(dev)
    params3 = draw_crop_flip(E, RandomCropFlip((th, tw)), (Hs, Ws), g).to(dev)
    table = ops.task_table([store], [store_y], [rows], [0], dev)
    gather64 = gather.long()
    x_mix = torch.empty((B + E, C, th, tw), device=dev)
    y_mix = torch.empty((B + E,), dtype=torch.int64, device=dev)
    ring_row0 = (N_TASKS - 1) * N_MEM
    geometry = (C, Hs, Ws, th, tw)
    row, frame = C * th * tw, C * Hs * Ws

    def fused():
        ops.rehearsal_assemble_resized_crop_flip(geometry, x, y, B, frames, src_idx, store, store_y, ring_row0, B, gather, params5,
                                                 x_mix, y_mix)

    def two_launch():
        ops.rehearsal_assemble_crop_flip(geometry, x, y, B, frames, src_idx, store, store_y, ring_row0, B, None, None, x_mix, y_mix)
        ops.gather_tasks_resized_crop_flip(table, geometry, gather64, params5, x_out=x_mix[B:], labels_out=y_mix[B:])

    def crop_fused():
        ops.rehearsal_assemble_crop_flip(geometry, x, y, B, frames, src_idx, store, store_y, ring_row0, B, gather, params3, x_mix, y_mix)

    fused()
    want, want_y = x_mix.clone(), y_mix.clone()
    x_mix.zero_()
    y_mix.zero_()
    two_launch()
    assert torch.equal(x_mix.view(torch.int32), want.view(torch.int32)) and torch.equal(y_mix, want_y)   # one device body: bitwise
    assert torch.equal(store[ring_row0:ring_row0 + B], frames.index_select(0, src_idx))
    window_elems = int((windows[:, 2].long() * windows[:, 3].long()).sum()) * C
    resampled = 4 * (2 * B * row + 2 * B * frame + window_elems + E * row)
    nbytes = {"fused": resampled, "two_launch": resampled, "crop_fused": 8 * (B * row + B * frame + E * row)}
    t = timed_together({"fused": fused, "two_launch": two_launch, "crop_fused": crop_fused}, a.iters, a.warmup, a.rounds)
    res = {"geometry": list(geometry), "current_rows": B, "ring_rows": B, "exemplar_rows": E,
           "mean_window": [float(windows[:, 2].float().mean()), float(windows[:, 3].float().mean())]}
    res.update({k: summary(t[k], nbytes[k]) for k in t})
    res["fused_over_two_launch"] = res["fused"]["median_us"] / res["two_launch"]["median_us"]
    res["fused_over_crop_fused"] = res["fused"]["median_us"] / res["crop_fused"]["median_us"]
    return res


def step_case(a, margin=8, hw=64):
    """RehearsalNet.observe_FT at task 10 in frame mode with the crop spec and with the resized spec, alternating inside every round."""
    from clsurvey_amd import models
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip
    from clsurvey_amd.methods.exemplar import BatchSource
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    B, E, chunk = step_shape()
    dev = "cuda"
    gen = torch.Generator().manual_seed(9)
    frames = torch.randn((2000, 3, hw + margin, hw + margin), generator=gen).to(dev)
    idx_host = torch.randperm(2000, generator=gen)[:B]
    src = BatchSource(frames, idx_host.to(dev), idx_host, None)
    x = frames[idx_host.to(dev), :, :hw, :hw].contiguous()
    y = torch.randint(0, 20, (B,), generator=gen).to(dev)
    ws = {}
    for mode, spec in (("crop", RandomCropFlip((hw, hw))), ("resized", RandomResizedCropFlip((hw, hw)))):
        torch.manual_seed(5)
        net = replace_head(models.parse_model_name("small_VGG9_cl_128_128", (hw, hw), 20), 20 * N_TASKS)
        w = RehearsalNet(net, 20 * N_TASKS, N_TASKS, [20] * N_TASKS, N_MEM, 1e-3, 0.0, False, B + E, (3, hw, hw), dev,
                         exemplar_transform=spec, frame_shape=(3, hw + margin, hw + margin))
        w.init_setup(lr=1e-3, weight_decay=0.0, n_append=E, chunk_size=chunk)
        w.store_x[:(N_TASKS - 1) * N_MEM].normal_()
        w.store_y[:(N_TASKS - 1) * N_MEM].random_(0, 20)
        w.observed_tasks, w.old_task, w.filled = list(range(N_TASKS - 1)), N_TASKS - 2, [N_MEM] * (N_TASKS - 1) + [0]
        ws[mode] = w
    random.seed(3)
    torch.manual_seed(4)

    def step(mode):
        ws[mode].observe_FT(x, N_TASKS - 1, y, source=src)

    for mode in ws:
        for _ in range(a.warmup):
            step(mode)
    torch.cuda.synchronize()
    out = {mode: [] for mode in ws}
    for _ in range(a.rounds):
        for mode in ws:
            t0 = time.perf_counter()
            for _ in range(a.iters):
                step(mode)
            torch.cuda.synchronize()
            out[mode].append((time.perf_counter() - t0) * 1e6 / a.iters)
    assert ws["crop"].last_path == ws["resized"].last_path == "fused"
    res = {"geometry": [3, hw + margin, hw + margin, hw, hw], "rows": B + E, "model": "small_VGG9_cl_128_128"}
    for mode, v in out.items():
        res[mode] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v)}
    res["resized_over_crop"] = res["resized"]["median_us"] / res["crop"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "72_to_64": kernel_case(3, 72, 64, a), "256_to_224": kernel_case(3, 256, 224, a),
           "step_72_to_64": step_case(a)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
