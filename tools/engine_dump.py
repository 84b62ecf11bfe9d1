#!/usr/bin/env python
"""Everything the plan executor (csrc/engine.hip) computes on fixed inputs, saved to one .npz: two builds compared bitwise across
processes.  CLHIP_LIB selects the build; the executor's switches (CLHIP_BS, CLHIP_WINO, CLHIP_EDGE_GRIDS, CLHIP_FC_TAIL,
CLHIP_WGRAD_OVERLAP, CLHIP_S2D) come from the environment, one process per setting.
    python tools/engine_dump.py out.npz               run the cases below on cuda:0
    python tools/engine_dump.py --compare a.npz b.npz every array np.array_equal (exit status 1 otherwise)
Cases: loss steps with and without gradients on the three bench-model plans; on small batches clhip_net_forward alone,
clhip_net_backward on its own after it (the executor prepares the backward weights itself there), a column-slice step, a
loss_segments step, an extra input gradient on a conv and on a Linear layer, the _BN and _DROP nets and a small AlexNet with seeded
dropout masks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        if not np.all(np.isfinite(A[k])):
            print("NOT FINITE", k)
            bad.append(k)
        elif not np.array_equal(A[k], B[k]):
            print("DIFFERENT ", k, "max |a - b| = %g" % np.abs(A[k].astype(np.float64) - B[k]).max())
            bad.append(k)
    print("%s | %s: %d arrays, %s" % (a, b, len(A.files), "all equal" if not bad else "%d DIFFER: %s" % (len(bad), bad)))
    return 1 if bad else 0


def main(path):
    import torch
    from clsurvey_amd import models, net, ops
    out = {}

    def keep(tag, **arrays):
        torch.cuda.synchronize()
        for k, v in arrays.items():
            out[tag + "_" + k] = v.detach().cpu().numpy().copy()

    def inputs(N, hw, classes=20, seed=5):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(N, 3, hw, hw, generator=g).cuda(), torch.randint(0, classes, (N,), generator=g).cuda()

    def engine(name, N, hw):
        torch.manual_seed(11)
        m = models.parse_model_name(name, (hw, hw), 20)
        return m, net.NetEngine(m, N, (3, hw, hw), "cuda")

    def seeded_masks(eng, N, seed=9):
        """nn.Dropout masks (p = 0.5) from a host generator: the same in every process"""
        eng.auto_dropout = False
        g = torch.Generator().manual_seed(seed)
        for li in sorted(eng.drops):
            eng.set_dropout(li, (torch.rand(N, eng.in_elems[li], generator=g) < 0.5).float().mul_(2.0).cuda())

    def step(eng, tag, x, y, kind="ce_mean", **kw):
        eng.arena.grad.zero_()
        loss, logits = eng.loss_step(x, y, kind, backward=True, want_logits=True, **kw)
        keep(tag, loss=loss, logits=logits, grad=eng.arena.grad)

    # the bench-model plans: loss steps with and without gradients
    for name, N, hw in (("small_VGG9_cl_128_128", 200, 64), ("small_VGG9_cl_128_128", 37, 64), ("base_VGG9_cl_512_512", 50, 64)):
        _, eng = engine(name, N, hw)
        x, y = inputs(N, hw)
        for kind in ("ce_mean", "ce_sum"):
            step(eng, "%s_%d_%s" % (name, N, kind), x, y, kind)
        loss, logits = eng.loss_step(x, y, "ce_mean", backward=False, want_logits=True)
        keep("%s_%d_nograd" % (name, N), loss=loss, logits=logits)
    # one small plan through every entry point
    N, hw = 24, 64
    _, eng = engine("small_VGG9_cl_128_128", N, hw)
    x, y = inputs(N, hw)
    logits = eng.forward(x)
    keep("fwd", logits=logits, prepared=eng.prepared_weights())
    g = torch.Generator().manual_seed(6)
    eng.arena.grad.zero_()
    eng.backward(x, torch.randn(N, 20, generator=g).cuda())
    keep("bwd_alone", grad=eng.arena.grad)
    ylocal = torch.remainder(y, 10)                     # labels count from the first column of a slice
    step(eng, "slice", x, ylocal, class_slice=(5, 15))
    step(eng, "mse", x, None, "mse_sum_zero")
    segs = ops.loss_segment_table([(0, 16, 10, 10, 1.0, 0), (16, 24, 0, 10, 0.5, 0)], "cuda")
    eng.arena.grad.zero_()
    loss, logits = eng.loss_step_segments(x, ylocal, segs, 2, want_logits=True)
    keep("segments", loss=loss, logits=logits, grad=eng.arena.grad)
    for layer in (3, 6):       # a conv layer (no one-grid backward, no fused un-pool for it) and the first Linear layer
        extra = torch.randn(N, eng.layer_input(layer, N).shape[1], generator=g).cuda()
        eng.set_input_grad(layer, extra)
        step(eng, "extra_grad_%d" % layer, x, y)
        eng.set_input_grad(layer, None)
    step(eng, "after_extra", x, y)
    # BatchNorm (training and running statistics) and Dropout variants, AlexNet geometry
    m, eng = engine("base_VGG9_cl_512_512_BN", N, hw)
    m.train()
    step(eng, "bn_train", x, y)
    keep("bn_train", **{"rmean%d" % li: bn.running_mean for li, bn in eng.bns.items()}, **{"rvar%d" % li: bn.running_var for li, bn in eng.bns.items()})
    m.eval()
    step(eng, "bn_eval", x, y)
    m, eng = engine("base_VGG9_cl_512_512_DROP", N, hw)
    m.train()
    seeded_masks(eng, N)
    step(eng, "drop", x, y, "ce_sum")
    torch.manual_seed(11)
    m = models.AlexNet(num_classes=10, widths=(8, 12, 16, 16, 8), fc=32, feat_hw=1)
    eng = net.NetEngine(m, 8, (3, 67, 67), "cuda")
    m.train()
    seeded_masks(eng, 8)
    x, y = inputs(8, 67, 10)
    step(eng, "alexnet", x, y)
    keep("alexnet_fwd", logits=eng.forward(x))
    np.savez(path, **out)
    print("saved", len(out))


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else main(sys.argv[1]))
