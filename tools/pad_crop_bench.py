"""One padded-crop batch of 200 out of 10 tasks, timed with HIP events (medians and spread over repeated rounds, the variants
alternating inside every round), at 3 x 64^2 -> 64^2 with pad 4 and at 3 x 224^2 -> 224^2 with pad 28, in all four padding
modes, on float and on byte frames:
  pad_kernel      clhip_gather_tasks_pad_crop_flip[_u8] out of the UNPADDED per-task frames: one launch
  prepadded       clhip_gather_tasks_crop_flip[_u8] out of frames padded once on the host side with torch.nn.functional.pad
                  (symmetric: the flip-and-concatenate form), (top + pad, left + pad, flip) rows: what a user does today, at
                  (1 + 2 pad / hw)^2 times the frames in HBM
  index_select    x.index_select(0, idx) + y.index_select(0, idx) on a merged float tensor of the OUTPUT's size: the floor for
                  the bytes written
The outputs of pad_kernel and prepadded are compared bitwise before anything is timed.  bytes = output read + written
(2 x B C th tw x 4); share_of_8TBps = bytes / time / 8e12 (the HBM figure of bench.py's roofline).  store_bytes: what the task
frames take in HBM, unpadded and pre-padded.
python tools/pad_crop_bench.py [--rounds 7] [--iters 20] [--warmup 5] [--out profiles/pad_crop_bench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from augment_bench import summary, timed_together  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL_BYTE = 128


def prepad(x, p, mode, fill):
    """x [n][C][H][W] padded by p on every side as torchvision's pad does it; bytes go through floats (exact) and back."""
    v = x.float() if x.dtype == torch.uint8 else x
    if mode == "constant":
        v = torch.stack([F.pad(v[:, c], (p, p, p, p), value=float(fill[c])) for c in range(v.shape[1])], 1)
    elif mode == "symmetric":
        v = torch.cat([v[..., :p].flip(-1), v, v[..., v.shape[-1] - p:].flip(-1)], -1)
        v = torch.cat([v[..., :p, :].flip(-2), v, v[..., v.shape[-2] - p:, :].flip(-2)], -2)
    else:
        v = F.pad(v, (p, p, p, p), mode="replicate" if mode == "edge" else "reflect")
    return v.to(x.dtype).contiguous()


def case(C, hw, p, n_per_task, a, T=10, B=200):
    from clsurvey_amd import ops
    from clsurvey_amd.data import PAD_MODES, RandomPadCropFlip, draw_pad_crop_flip, norm_lut
    dev = "cuda"
    gen = torch.Generator().manual_seed(1)
    ys = [torch.randint(0, 20, (n_per_task,), device=dev) for _ in range(T)]
    cum = [n_per_task * (j + 1) for j in range(T)]
    shifts = [20 * j for j in range(T)]
    merged_y = torch.cat([y + s for y, s in zip(ys, shifts)])
    small = torch.randn((T * n_per_task, C, hw, hw), device=dev)      # index_select: a dataset of the output's size
    idx = torch.randperm(T * n_per_task, generator=gen)[:B].to(dev)
    lut = norm_lut(torch.tensor(MEAN[:C]), torch.tensor(STD[:C])).to(dev)
    geometry, padded_geometry = (C, hw, hw, hw, hw), (C, hw + 2 * p, hw + 2 * p, hw, hw)
    out_bytes = 2 * B * C * hw * hw * 4
    res = {"geometry": list(geometry), "pad": p, "tasks": T, "batch": B, "frames_per_task": n_per_task}
    for kind in ("float", "byte"):
        if kind == "float":
            xs = [torch.randn((n_per_task, C, hw, hw), device=dev) for _ in range(T)]
            fill_src = [0.0] * C                                      # the fill in the domain of the stored frames
            fill = torch.zeros((C,), device=dev)
        else:
            xs = [torch.randint(0, 256, (n_per_task, C, hw, hw), device=dev, dtype=torch.uint8) for _ in range(T)]
            fill_src = [FILL_BYTE] * C
            fill = lut[:, FILL_BYTE].contiguous()
        table = ops.task_table(xs, ys, cum, shifts, dev)
        res[kind] = {"store_bytes": {"unpadded": sum(x.numel() * x.element_size() for x in xs)}}
        for mode in PAD_MODES:
            params = draw_pad_crop_flip(B, RandomPadCropFlip((hw, hw), p, padding_mode=mode), (hw, hw), gen)
            shifted = (params[:, :3] + torch.tensor([p, p, 0], dtype=torch.int32)).contiguous().to(dev)
            params = params.to(dev)
            padded = [prepad(x, p, mode, fill_src) for x in xs]
            padded_table = ops.task_table(padded, ys, cum, shifts, dev)
            res[kind]["store_bytes"]["prepadded"] = sum(x.numel() * x.element_size() for x in padded)
            if kind == "float":
                def pad_kernel():
                    return ops.gather_tasks_pad_crop_flip(table, geometry, mode, (p, p, p, p), fill, idx, params)

                def prepadded():
                    return ops.gather_tasks_crop_flip(padded_table, padded_geometry, idx, shifted)
            else:
                def pad_kernel():
                    return ops.gather_tasks_pad_crop_flip_u8(table, geometry, mode, (p, p, p, p), fill, lut, idx, params)

                def prepadded():
                    return ops.gather_tasks_crop_flip_u8(padded_table, padded_geometry, lut, idx, shifted)

            def index_select():
                return small.index_select(0, idx), merged_y.index_select(0, idx)

            got, want = pad_kernel(), prepadded()
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), (kind, mode)
            t = timed_together({"pad_kernel": pad_kernel, "prepadded": prepadded, "index_select": index_select},
                               a.iters, a.warmup, a.rounds)
            r = {name: summary(v, out_bytes) for name, v in t.items()}
            r["pad_kernel_over_prepadded"] = r["pad_kernel"]["median_us"] / r["prepadded"]["median_us"]
            r["pad_kernel_over_index_select"] = r["pad_kernel"]["median_us"] / r["index_select"]["median_us"]
            res[kind][mode] = r
            del padded, padded_table
        sb = res[kind]["store_bytes"]
        sb["saved_share"] = 1.0 - sb["unpadded"] / sb["prepadded"]
        del xs, table
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"64_pad_4": case(3, 64, 4, 2000, a), "224_pad_28": case(3, 224, 28, 400, a)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
