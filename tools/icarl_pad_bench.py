"""The batch assembly of a task-10 iCaRL step on RandomCrop(64, padding=4) tasks (200 current rows, the exemplar rows
exemplar_split gives 'icarl' -- the full-memory ratio -- for 450 memories per task and 8000 training images, target rows of 200
outputs, as tools/icarl_augment_bench.py sizes them), timed with HIP events (medians and spread over repeated rounds, the variants
alternating inside every round), at 3 x 64^2, pad 4, in all four padding modes, on an fp32 and on a byte exemplar store:
  pad_assembly    clhip_icarl_assemble_pad_crop_flip[_u8] on a store of the UNPADDED 64^2 frames: current rows, exemplars padded,
                  cropped and mirrored, their target rows; one launch
  prepadded       clhip_icarl_assemble_crop_flip[_u8] on a store of frames padded once on the host to 72^2, (top + pad,
                  left + pad, flip) rows, same current, exemplar and target rows: what a user does without the padded entry, at
                  (1 + 2 pad / hw)^2 times the store in HBM
x_mix, y_mix and t_mix of the two are compared bitwise before anything is timed.  bytes = read + written of every row a variant
moves; share_of_8TBps = bytes / time / 8e12 (the HBM figure of bench.py's roofline).  store_bytes: what the exemplar store of
10 x 450 frames takes in HBM, unpadded and pre-padded.
python tools/icarl_pad_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/icarl_pad_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from augment_bench import summary, timed_together  # noqa: E402
from icarl_augment_bench import N_MEM, N_TASKS, NC, step_shape  # noqa: E402
from pad_crop_bench import FILL_BYTE, MEAN, STD, prepad  # noqa: E402


def case(C, hw, p, a):
    from clsurvey_amd import ops
    from clsurvey_amd.data import PAD_MODES, RandomPadCropFlip, draw_pad_crop_flip, norm_lut
    B, E, _ = step_shape()
    dev = "cuda"
    rows, n_out = N_TASKS * N_MEM, NC * N_TASKS
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((B, C, hw, hw), device=dev)
    y = torch.randint(0, NC, (B,), device=dev)
    store_t = torch.randn((rows, n_out), device=dev)
    gather = torch.randperm((N_TASKS - 1) * N_MEM, generator=gen)[:E].to(torch.int32).to(dev)    # rows of the nine past tasks
    lut = norm_lut(torch.tensor(MEAN[:C]), torch.tensor(STD[:C])).to(dev)
    geometry, padded_geometry = (C, hw, hw, hw, hw), (C, hw + 2 * p, hw + 2 * p, hw, hw)
    pads = (p, p, p, p)
    row = C * hw * hw
    res = {"geometry": list(geometry), "pad": p, "current_rows": B, "exemplar_rows": E, "n_outputs": n_out, "store_rows": rows}
    for kind in ("float", "byte"):
        if kind == "float":
            store = torch.randn((rows, C, hw, hw), device=dev)
            fill_src, fill, table, es = [0.0] * C, torch.zeros((C,), device=dev), (), 4
            pad_entry, crop_entry = ops.icarl_assemble_pad_crop_flip, ops.icarl_assemble_crop_flip
        else:
            store = torch.randint(0, 256, (rows, C, hw, hw), device=dev, dtype=torch.uint8)
            fill_src, fill, table, es = [FILL_BYTE] * C, lut[:, FILL_BYTE].contiguous(), (lut,), 1
            pad_entry, crop_entry = ops.icarl_assemble_pad_crop_flip_u8, ops.icarl_assemble_crop_flip_u8
        res[kind] = {"store_bytes": {"unpadded": store.numel() * store.element_size()}}
        # bytes read + written: current rows, exemplar rows (their source bytes counted at the output's size), target rows
        nbytes = 8 * B * row + (4 + es) * E * row + 8 * E * n_out
        for mode in PAD_MODES:
            params = draw_pad_crop_flip(E, RandomPadCropFlip((hw, hw), p, padding_mode=mode), (hw, hw), gen)
            shifted = (params[:, :3] + torch.tensor([p, p, 0], dtype=torch.int32)).contiguous().to(dev)
            params = params.to(dev)
            store_p = prepad(store, p, mode, fill_src)
            res[kind]["store_bytes"]["prepadded"] = store_p.numel() * store_p.element_size()
            xm, xm_p = (torch.zeros((B + E, C, hw, hw), device=dev) for _ in range(2))
            ym, ym_p = (torch.full((B + E,), -5, dtype=torch.int64, device=dev) for _ in range(2))
            tm, tm_p = (torch.zeros((B + E, n_out), device=dev) for _ in range(2))

            def pad_assembly():
                pad_entry(geometry, mode, pads, fill, *table, x, y, B, store, gather, params, store_t, xm, ym, tm)

            def prepadded():
                crop_entry(padded_geometry, *table, x, y, B, store_p, gather, shifted, store_t, xm_p, ym_p, tm_p)

            pad_assembly()
            prepadded()
            assert torch.equal(xm.view(torch.int32), xm_p.view(torch.int32)) and torch.equal(ym, ym_p), (kind, mode)
            assert torch.equal(tm.view(torch.int32), tm_p.view(torch.int32)), (kind, mode)
            assert torch.equal(tm[B:], store_t.index_select(0, gather.long())) and int(ym[B:].abs().sum()) == 0
            t = timed_together({"pad_assembly": pad_assembly, "prepadded": prepadded}, a.iters, a.warmup, a.rounds)
            r = {name: summary(v, nbytes) for name, v in t.items()}
            r["pad_assembly_over_prepadded"] = r["pad_assembly"]["median_us"] / r["prepadded"]["median_us"]
            res[kind][mode] = r
            del store_p
        sb = res[kind]["store_bytes"]
        sb["saved_share"] = 1.0 - sb["unpadded"] / sb["prepadded"]
        del store
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "64_pad_4": case(3, 64, 4, a)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
