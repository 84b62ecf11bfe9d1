"""The batch assembly of a task-10 iCaRL step on AUGMENTED tasks (200 current rows, the exemplar rows exemplar_split gives 'icarl'
-- the full-memory ratio -- for 450 memories per task and 8000 training images, target rows of 200 outputs), timed with HIP events
(medians and spread over repeated rounds, the variants alternating inside every round), at 3 x 72^2 -> 64^2 and 3 x 256^2 ->
224^2, for RandomCropFlip and RandomResizedCropFlip draws, fp32 and uint8 stores:
  single          clhip_icarl_assemble_*: current rows, exemplar windows and their target rows in ONE launch
  composition     the entries it replaces: clhip_rehearsal_assemble_* with ring_rows = 0 (current rows + exemplar windows), then
                  clhip_rehearsal_assemble over the target rows
bytes = read + written of every row a variant moves (a resized window counted at its own size, a byte at its own size);
share_of_8TBps = bytes / time / 8e12 (the HBM figure of bench.py's roofline).
Then the WHOLE step of IcarlNet.observe at 64^2 (host plan and draws, upload, assembly, one fused engine pass of
small_VGG9_cl_128_128 with the CE + distillation loss, SGD) in crop mode, in frame mode and in resized frame mode, host clock
around a device synchronise.
python tools/icarl_augment_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/icarl_augment_bench.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.augment_bench import summary, timed_together  # noqa: E402

N_TASKS, N_MEM, N_TRAIN, BATCH, NC = 10, 450, 8000, 200, 20


def step_shape():
    """(current rows, exemplar rows, total_batch_size) of a task-10 iCaRL step, as gem_main.exemplar_split shares them out."""
    from clsurvey_amd.methods.gem_main import exemplar_split
    args = argparse.Namespace(method="icarl", n_memories=N_MEM, task_idx=N_TASKS - 1, n_tasks=N_TASKS, batch_size=BATCH)
    exemplar_split(args, {"train": N_TRAIN})
    return BATCH, args.n_exemplars_to_append_per_batch, args.total_batch_size


def kernel_case(C, Hs, th, resized, byte, a):
    from clsurvey_amd import _lib, ops
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip, draw_crop_flip, draw_resized_crop_flip, norm_lut
    B, E, _ = step_shape()
    Ws, tw = Hs, th
    dev = "cuda"
    rows, n_out = N_TASKS * N_MEM, NC * N_TASKS
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, C, th, tw), device=dev)
    y = torch.randint(0, NC, (B,), device=dev)
    if byte:
        store = torch.randint(0, 256, (rows, C, Hs, Ws), dtype=torch.uint8, device=dev)
        lut = (norm_lut(torch.full((C,), 0.5), torch.full((C,), 0.25)).to(dev),)
    else:
        store, lut = torch.randn((rows, C, Hs, Ws), device=dev), ()
    store_t = torch.randn((rows, n_out), device=dev)
    zero_lab = torch.zeros((rows,), dtype=torch.int64, device=dev)
    scratch = torch.empty((E,), dtype=torch.int64, device=dev)
    gather = torch.randperm((N_TASKS - 1) * N_MEM, generator=g)[:E].to(torch.int32).to(dev)      # rows of the nine past tasks
    if resized:
        windows = draw_resized_crop_flip(E, RandomResizedCropFlip((th, tw)), (Hs, Ws), g)
        window_elems = int((windows[:, 2].long() * windows[:, 3].long()).sum()) * C
    else:
        windows = draw_crop_flip(E, RandomCropFlip((th, tw)), (Hs, Ws), g)
        window_elems = E * C * th * tw
    params = windows.to(dev)
    x_mix = torch.empty((B + E, C, th, tw), device=dev)
    y_mix = torch.empty((B + E,), dtype=torch.int64, device=dev)
    t_mix = torch.zeros((B + E, n_out), device=dev)
    geometry = (C, Hs, Ws, th, tw)
    name = "%scrop_flip%s" % ("resized_" if resized else "", "_u8" if byte else "")
    single_entry, parent_entry = getattr(ops, "icarl_assemble_" + name), getattr(ops, "rehearsal_assemble_" + name)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def single():
        single_entry(geometry, *lut, x, y, B, store, gather, params, store_t, x_mix, y_mix, t_mix)

    def composition():
        parent_entry(geometry, *lut, x, y, B, None, None, store, zero_lab, 0, 0, gather, params, x_mix, y_mix)
        _lib.check(L.clhip_rehearsal_assemble(None, None, 0, n_out, store_t.data_ptr(), zero_lab.data_ptr(), rows, 0, 0,
                                              gather.data_ptr(), E, t_mix[B:].data_ptr(), scratch.data_ptr(), stream),
                   "clhip_rehearsal_assemble")

    single()
    want = (x_mix.clone(), y_mix.clone(), t_mix.clone())
    x_mix.zero_()
    y_mix.fill_(-5)
    t_mix.zero_()
    composition()
    assert torch.equal(x_mix.view(torch.int32), want[0].view(torch.int32)) and torch.equal(y_mix, want[1])       # one device body: bitwise
    assert torch.equal(t_mix, want[2]) and torch.equal(t_mix[B:], store_t.index_select(0, gather.long()))
    row = C * th * tw
    nbytes = 8 * B * row + window_elems * (1 if byte else 4) + 4 * E * row + 8 * E * n_out
    t = timed_together({"single": single, "composition": composition}, a.iters, a.warmup, a.rounds)
    res = {"geometry": list(geometry), "kind": name, "current_rows": B, "exemplar_rows": E, "n_outputs": n_out}
    res.update({k: summary(t[k], nbytes) for k in t})
    res["single_over_composition"] = res["single"]["median_us"] / res["composition"]["median_us"]
    return res


def step_case(a, margin=8, hw=64):
    """IcarlNet.observe at task 10 in crop mode, in frame mode and in resized frame mode, alternating inside every round."""
    from clsurvey_amd import models
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip
    from clsurvey_amd.methods.exemplar import BatchSource
    from clsurvey_amd.methods.icarl import IcarlNet
    B, E, total = step_shape()
    dev = "cuda"
    gen = torch.Generator().manual_seed(9)
    frames = torch.randn((2000, 3, hw + margin, hw + margin), generator=gen).to(dev)
    idx_host = torch.randperm(2000, generator=gen)[:B]
    src = BatchSource(frames, idx_host.to(dev), idx_host, None)
    x = frames[idx_host.to(dev), :, :hw, :hw].contiguous()
    y = torch.randint(0, NC, (B,), generator=gen).to(dev)
    count = N_TASKS * N_MEM // (NC * (N_TASKS - 1))                            # K/m after the ninth manage_memory
    ws = {}
    for mode, spec in (("crop", None), ("frames", RandomCropFlip((hw, hw))), ("resized_frames", RandomResizedCropFlip((hw, hw)))):
        torch.manual_seed(5)
        kw = {} if spec is None else dict(exemplar_transform=spec, frame_shape=(3, hw + margin, hw + margin))
        w = IcarlNet(models.parse_model_name("small_VGG9_cl_128_128", (hw, hw), NC), NC * N_TASKS, N_TASKS, [NC] * N_TASKS, N_MEM, 1e-3,
                     0.0, 1.0, B + E, (3, hw, hw), dev, **kw)
        w.init_setup(lr=1e-3, weight_decay=0.0, memory_strength=1.0, n_append=E, chunk_size=B - E, total_batch_size=total)
        w.exemplar_count, w.class_len = count, [count] * (NC * (N_TASKS - 1))
        w.store_x.normal_()
        w.store_t.normal_()
        w.observed_tasks, w.old_task = list(range(N_TASKS)), N_TASKS - 1
        ws[mode] = w
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(4)

    def step(mode):
        ws[mode].observe(x, N_TASKS - 1, y, **({} if mode == "crop" else {"source": src}))

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
    assert all(w.last_path == "fused" for w in ws.values())
    res = {"geometry": [3, hw + margin, hw + margin, hw, hw], "rows": B + E, "model": "small_VGG9_cl_128_128"}
    for mode, v in out.items():
        res[mode] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v)}
    res["frames_over_crop"] = res["frames"]["median_us"] / res["crop"]["median_us"]
    res["resized_frames_over_crop"] = res["resized_frames"]["median_us"] / res["crop"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    for Hs, th in ((72, 64), (256, 224)):
        for resized in (False, True):
            for byte in (False, True):
                res["kernels"].append(kernel_case(3, Hs, th, resized, byte, a))
    res["step_72_to_64"] = step_case(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
