"""The frame-mode batch assembly of the exemplar wrappers with a BYTE store against the same launch with an fp32 store, timed with
HIP events (medians and spread over repeated rounds, the two entries alternating inside every round), at 3 x 72^2 -> 64^2 and
3 x 256^2 -> 224^2, one process:
  step       a rehearsal step: 160 current rows, 160 ring rows out of the loader's frames, 40 exemplars cropped out of the store
             clhip_rehearsal_assemble_crop_flip_u8 against clhip_rehearsal_assemble_crop_flip
  ring_only  GEM's fill_buffer: the 160 ring rows alone (no x_mix, no table)
The fp32 side works on the decoded twins of the byte frames; stores, labels and batches of a pair are compared bitwise before
anything is timed.  moved_bytes = what a launch reads and writes at the least (current rows and exemplar rows: fp32 out; ring
rows: a frame in and out; exemplar windows: th x tw elements in); resident_bytes = what the store takes in HBM in either form.
python tools/u8_exemplar_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--frames 2000] [--store_rows 1024] [--out profiles/u8_exemplar_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
B, RING, E = 160, 160, 40


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


def summary(v, moved_bytes):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v), "moved_bytes": moved_bytes}


def case(C, Hs, th, a):
    from clsurvey_amd import ops
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, draw_crop_flip
    Ws, tw = Hs, th
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1)
    n, rows = a.frames, a.store_rows
    y = torch.randint(0, 20, (B,), device=dev, generator=gen)
    src_b = ByteTaskDataset(torch.randint(0, 256, (n, C, Hs, Ws), device=dev, dtype=torch.uint8, generator=gen),
                            torch.zeros((n,), dtype=torch.int64, device=dev), [], MEAN[:C], STD[:C])
    store_b = ByteTaskDataset(torch.randint(0, 256, (rows, C, Hs, Ws), device=dev, dtype=torch.uint8, generator=gen),
                              torch.randint(0, 20, (rows,), device=dev, generator=gen), [], MEAN[:C], STD[:C])
    src_f, store_f = src_b.decoded().x, store_b.decoded().x
    sy_b, sy_f = store_b.y.clone(), store_b.y.clone()
    lut = src_b.lut().to(dev)
    g = torch.Generator().manual_seed(1)
    src_idx = torch.randperm(n, generator=g)[:RING].to(dev)
    row0 = rows - RING                                             # the ring rows are the last ones, the exemplars come from before
    gather = torch.randperm(row0, generator=g)[:E].to(torch.int32).to(dev)
    params = draw_crop_flip(E, RandomCropFlip((th, tw)), (Hs, Ws), g).to(dev)
    geometry = (C, Hs, Ws, th, tw)
    x = torch.randn((B, C, th, tw), device=dev, generator=gen)
    xm_b, xm_f = (torch.empty((B + E, C, th, tw), device=dev) for _ in range(2))
    ym_b, ym_f = (torch.empty((B + E,), dtype=torch.int64, device=dev) for _ in range(2))
    pairs = {
        "step": (lambda: ops.rehearsal_assemble_crop_flip_u8(geometry, lut, x, y, B, src_b.x, src_idx, store_b.x, sy_b, row0, RING,
                                                             gather, params, xm_b, ym_b),
                 lambda: ops.rehearsal_assemble_crop_flip(geometry, x, y, B, src_f, src_idx, store_f, sy_f, row0, RING, gather, params,
                                                          xm_f, ym_f)),
        "ring_only": (lambda: ops.rehearsal_assemble_crop_flip_u8(geometry, None, None, y, B, src_b.x, src_idx, store_b.x, sy_b, row0,
                                                                  RING, None, None, None, None),
                      lambda: ops.rehearsal_assemble_crop_flip(geometry, None, y, B, src_f, src_idx, store_f, sy_f, row0, RING, None,
                                                               None, None, None)),
    }
    row, frame = C * th * tw, C * Hs * Ws
    moved = {"step": lambda s: 8 * B * row + 2 * s * RING * frame + (s + 4) * E * row, "ring_only": lambda s: 2 * s * RING * frame}
    res = {"geometry": list(geometry), "batch": B, "ring_rows": RING, "exemplars": E, "source_frames": n, "store_rows": rows,
           "resident_bytes": {"u8": store_b.x.numel(), "fp32": 4 * store_f.numel()}}
    for name, (u8, fp32) in pairs.items():
        u8()
        fp32()
        torch.cuda.synchronize()
        table = lut.cpu()
        dec = torch.stack([table[c].to(dev)[store_b.x[row0:, c].long()] for c in range(C)], 1)
        assert torch.equal(dec.view(torch.int32), store_f[row0:].view(torch.int32)) and torch.equal(sy_b, sy_f), name
        assert torch.equal(store_b.x[row0:], src_b.x[src_idx]), name
        if name == "step":
            assert torch.equal(xm_b.view(torch.int32), xm_f.view(torch.int32)) and torch.equal(ym_b, ym_f), name
        t = timed_together({"u8": u8, "fp32": fp32}, a.iters, a.warmup, a.rounds)
        res[name] = {"u8": summary(t["u8"], moved[name](1)), "fp32": summary(t["fp32"], moved[name](4))}
        res[name]["u8_over_fp32"] = res[name]["u8"]["median_us"] / res[name]["fp32"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2000, help="frames of the loader the ring rows come from")
    ap.add_argument("--store_rows", type=int, default=1024, help="rows of the exemplar store")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name, (C, Hs, th) in (("72_to_64", (3, 72, 64)), ("256_to_224", (3, 256, 224))):
        res[name] = case(C, Hs, th, a)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
