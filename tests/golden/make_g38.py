"""G38: PathNet forward / train_epoch fixture from the reference's UNCHANGED networks/vgg_pathnet.py and
approaches/pathnet.py (dev container only, CPU).

For every case of g38_common.CASES (two (N, M) settings; a plain path, a path with a duplicated module, a path at t = 1
over a frozen task-0 best path) it records the logits of Net.forward(x, t, path) in eval mode, the CE loss, every
parameter that moved in one Appr.train_epoch over three batches (40, 40, 7) with momentum, weight decay and clipgrad, and
the names of those that did not move.  The same run in float64 gives the reference's own fp32-vs-fp64 gap.  Start weights
and inputs come from g38_common and are not recorded.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "harness"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import harness  # noqa: E402

torch = harness.install()
if not hasattr(np, "int"):
    np.int = int                                   # vgg_pathnet.py:94 predates NumPy 1.24
import models.VGGSlim as V  # noqa: E402
import g38_common as G  # noqa: E402


def build(setting, dtype):
    import methods.HAT.networks.vgg_pathnet as NET
    N, M = G.SETTINGS[setting]
    V.cfg["tiny_VGG9"] = G.CFG
    raw = V.VGGSlim(config="tiny_VGG9", num_classes=G.NCLS, classifier_inputdim=64 * 2 * 2, classifier_dim1=G.FC[0],
                    classifier_dim2=G.FC[1])
    args = types.SimpleNamespace(parameter=[N, M, 1], weight_decay=G.WD)
    net = NET.Net(raw, (3, G.HW, G.HW), [(t, G.NCLS) for t in range(G.NTASKS)], args=args)
    w = G.start_weights(setting)
    own = [(n, p) for n, p in net.named_parameters() if not n.startswith("initial_model.")]
    assert [n for n, _ in own] == [n for n, _ in G.shapes(N, M)]
    with torch.no_grad():
        for n, p in own:
            assert tuple(p.shape) == w[n].shape, n
            p.copy_(torch.from_numpy(w[n]))
    return net.to(dtype), args, [n for n, _ in own]


def run(case, dtype):
    import methods.HAT.approaches.pathnet as AP
    c = G.CASES[case]
    net, args, names = build(c["setting"], dtype)
    path = np.array(c["path"])
    if c["best0"] is not None:
        net.bestPath[0] = np.array(c["best0"])
    data = [(torch.from_numpy(x).to(dtype), torch.from_numpy(y)) for x, y in G.batches(case)]
    net.eval()
    with torch.no_grad():
        logits = net.forward(data[0][0], c["t"], path)
        loss = torch.nn.functional.cross_entropy(logits, data[0][1])
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    appr = AP.Appr(net, tempfile.gettempdir(), nepochs=1, sbatch=40, lr=G.LR, clipgrad=c["clipgrad"], args=args)
    net.unfreeze_path(c["t"], path)
    trainable = [n for n, p in net.named_parameters() if p.requires_grad and not n.startswith("initial_model.")]
    appr.optimizer = appr._get_optimizer(G.LR)
    norms = []
    clip = torch.nn.utils.clip_grad_norm

    def spy(params, max_norm):
        total = clip(params, max_norm)
        norms.append(float(total))
        return total
    torch.nn.utils.clip_grad_norm = spy
    try:
        appr.train_epoch(c["t"], data, path, use_gpu=False)
    finally:
        torch.nn.utils.clip_grad_norm = clip
    assert len(norms) == len(data)
    assert all((v > c["clipgrad"]) == c["clips"] for v in norms), (case, norms)
    after = {n: p.detach().clone() for n, p in net.named_parameters() if not n.startswith("initial_model.")}
    moved = [n for n in names if not torch.equal(after[n], start[n])]
    for n, p in net.named_parameters():
        if n.startswith("initial_model."):
            assert torch.equal(p.detach(), start[n])
    return dict(logits=logits, loss=loss, after=after, moved=moved, trainable=trainable, norms=norms)


def main():
    out = {"hyper": np.array([G.LR, G.MOMENTUM, G.WD]), "cases": np.array(sorted(G.CASES))}
    for case in sorted(G.CASES):
        r32, r64 = run(case, torch.float32), run(case, torch.float64)
        assert r32["moved"] == r64["moved"] == r32["trainable"], case        # every trainable module is in the path
        out[case + "_logits"] = r32["logits"].numpy()
        out[case + "_loss"] = np.array([float(r32["loss"])], dtype=np.float32)
        out[case + "_moved"] = np.array(r32["moved"])
        out[case + "_unmoved"] = np.array([n for n in r32["after"] if n not in r32["moved"]])
        out[case + "_norms"] = np.array(r64["norms"])
        for n in r32["moved"]:
            out[case + "_p_" + n] = r32["after"][n].numpy()

        def rel(a, b):
            return float((a.double() - b).abs().max() / b.abs().max())
        out[case + "_gap"] = np.array([rel(r32["logits"], r64["logits"]), rel(r32["loss"].view(1), r64["loss"].view(1)),
                                       max(rel(r32["after"][n], r64["after"][n]) for n in r32["moved"])])
        print(case, "logit max %.2f loss %.3f" % (float(r64["logits"].abs().max()), float(r64["loss"])), "norms", ["%.3f" % v for v in r64["norms"]], "moved", len(r32["moved"]), "gap", out[case + "_gap"])
    dst = os.path.join(HERE, "G38_pathnet_step.npz")
    np.savez_compressed(dst, **out)
    print(os.path.getsize(dst) // 1024, "KiB")


if __name__ == "__main__":
    main()
