"""PathNet on the device: the three kernels of csrc/pathnet.hip against tests/pathnet_ref.py (which the reference's G38
pins on CPU, tests/test_pathnet_cpu.py), and PathEngine's forward / three training steps against G38 itself."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import g38_common as G  # noqa: E402
import pathnet_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
MAXPOOL = [0, 1, 3, 5]
EPS = 2.0 ** -24                              # unit round-off of fp32


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def build(setting, best0=None, max_batch=40):
    from clsurvey_amd import models
    from clsurvey_amd.methods import pathnet as PN
    N, M = G.SETTINGS[setting]
    raw = models.VGGSlim(cfg=G.CFG, num_classes=G.NCLS, classifier_inputdim=64 * 2 * 2, classifier_dim1=G.FC[0],
                         classifier_dim2=G.FC[1])
    net = PN.PathNet(raw, (3, G.HW, G.HW), [(t, G.NCLS) for t in range(G.NTASKS)], [N, M])
    start = {n: torch.from_numpy(v) for n, v in G.start_weights(setting).items()}
    with torch.no_grad():
        for n, p in net.named_parameters():
            if not n.startswith("initial_model."):
                p.copy_(start[n])
    if best0 is not None:
        net.bestPath[0] = np.array(best0)
    return net, PN.PathEngine(net, max_batch, (3, G.HW, G.HW), dev()), start


def own_state(net):
    return {n: p.detach().cpu().clone() for n, p in net.named_parameters() if not n.startswith("initial_model.")}


def packed_of(eng):
    """[(weight, bias)] of the packed arena on the host, shaped as pathnet_ref.pack shapes them."""
    ps = list(eng.holder.packed)
    return [(ps[i].detach().cpu(), ps[i + 1].detach().cpu()) for i in range(0, len(ps), 2)]


PACK_CASES = [("a", G.A_PLAIN, 0), ("a", G.CASES["a_dup"]["path"], 0), ("b", G.B_PLAIN, 0), ("b", G.CASES["b_dup"]["path"], 0),
              ("b", [[0, -1, 4], [1, 3, -1], [-1, 0, 2], [2, 1, 3], [0, -1, 4], [3, 2, 1], [1, 0, -1], [2, 3, 4]], 0)]


@pytest.mark.parametrize("setting,path,t", PACK_CASES)
def test_pack_is_bitwise_the_restatement(setting, path, t):
    N, M = G.SETTINGS[setting]
    net, eng, start = build(setting)
    eng.P.theta.fill_(float("nan"))                       # every packed element, padding included, must be written
    eng.set_path(np.array(path), t)
    ref = PR.pack(start, np.array(path), N)
    got = packed_of(eng)
    assert len(got) == len(ref) == G.LAYERS + 1
    for (w, b), (rw, rb) in zip(got, ref):
        assert w.shape == rw.shape and torch.equal(w, rw) and torch.equal(b, rb)
    c = int(G.CFG[0] / M)                                 # the padded rows and columns of the second layer are exactly 0
    w, b = got[1]
    assert w.shape[0] % 32 == 0 and float(w[N * c:].abs().max()) == 0 and float(w[:, N * c:].abs().max()) == 0
    assert float(b[N * c:].abs().max()) == 0
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in net.own_parameters()]).cpu(),
                       torch.cat([start[n].reshape(-1) for n, _ in G.shapes(N, M)]))          # the modules are only read


FOLD_CASES = [("a", "a_plain"), ("a", "a_dup"), ("a", "a_t1"), ("b", "b_dup"), ("b", "b_t1")]


def random_packed_grad(eng, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(eng.P.numel, generator=gen) * scale
    eng.P.grad.copy_(g)
    ps = list(eng.holder.packed)
    return [(ps[i].grad.detach().cpu().clone(), ps[i + 1].grad.detach().cpu().clone()) for i in range(0, len(ps), 2)]


def named_grads(net):
    return {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters() if not n.startswith("initial_model.")}


@pytest.mark.parametrize("setting,case", FOLD_CASES)
def test_fold_matches_fp64_and_leaves_frozen_modules_alone(setting, case):
    """Each folded value is an fp32 sum of T terms in a fixed order (T = N replicas x the slots that hold the module, so N,
    or 2N for a module that sits twice in its layer): |error| <= (T - 1) * 2^-24 * sum |terms| (Higham, recursive
    summation).  The workspace holds the fp64 sum of squares of what was written."""
    c = G.CASES[case]
    N, M = G.SETTINGS[setting]
    path = np.array(c["path"])
    net, eng, start = build(setting, c["best0"])
    eng.set_path(path, c["t"])
    pg = random_packed_grad(eng, 11)
    SENT = -12345.5
    eng.A.grad.fill_(SENT)
    eng.fold()
    torch.cuda.synchronize()
    got = named_grads(net)
    train = PR.trainable(net.bestPath, c["t"], path, M)
    ref = PR.fold(pg, start, path, N, train, dtype=torch.float64)
    mag = PR.fold([(w.abs(), b.abs()) for w, b in pg], start, path, N, train, dtype=torch.float64)
    assert sorted(ref) == sorted(str(n) for n in np.load(os.path.join(HERE, "golden", "G38_pathnet_step.npz"))[case + "_moved"])
    lay, _ = PR.layers(start)
    sumsq_ref, sumsq_bound, sumsq_got = 0.0, 0.0, 0.0
    for li, mod in PR.active(start, path, N, train):
        slots = 1 if li == G.LAYERS else int((path[li] == mod).sum())
        for name in PR.names(lay[li], mod):
            T = slots * (1 if (li == 0 or name.endswith("bias")) else N)
            err = (got[name].double() - ref[name]).abs()
            assert bool((err <= (T - 1) * EPS * mag[name] + 1e-300).all()), (name, T, float(err.max()))
            sumsq_ref += float((ref[name] ** 2).sum())
            sumsq_got += float((got[name].double() ** 2).sum())
            sumsq_bound += float((2 * (T - 1) * EPS * mag[name] * ref[name].abs()).sum())
    for name, g in got.items():
        if name not in ref:
            assert bool((g == SENT).all()), name                 # frozen or off the path: never written
    ws = eng._ws.view(torch.float64).cpu()
    total = float(ws.sum())
    print("%s: sum of squares %.9e (fp64 fold %.9e, bound %.2e)" % (case, total, sumsq_ref, sumsq_bound))
    assert abs(total - sumsq_got) <= 1e-12 * sumsq_got
    assert abs(total - sumsq_ref) <= sumsq_bound + 1e-12 * sumsq_ref


@pytest.mark.parametrize("setting,case,clip", [("a", "a_t1", 1000.0), ("a", "a_dup", 2.0), ("b", "b_t1", 2.0), ("b", "b_dup", 1000.0)])
def test_sgd_matches_torch_clip_and_sgd(setting, case, clip):
    """One and two steps of clip_grad_norm + torch.optim.SGD(momentum, weight_decay) on CPU from the gradients the fold left;
    1e-6 of each tensor's scale, as the other parameter-update kernels are held to (tests/test_gpu_parity.py)."""
    from clsurvey_amd.methods import pathnet as PN
    c = G.CASES[case]
    N, M = G.SETTINGS[setting]
    path = np.array(c["path"])
    runs = []
    for rep in range(2):                                         # two runs from one state agree bitwise
        net, eng, start = build(setting, c["best0"])
        eng.set_path(path, c["t"])
        opt = PN.PathSGD(eng, G.LR, G.MOMENTUM, G.WD)
        opt.buf.fill_(float("nan"))                              # first step: the momentum buffer is written, never read
        cpu = {n: torch.nn.Parameter(v.clone()) for n, v in start.items()}
        ref_opt, seen = None, []
        for step in range(2):
            random_packed_grad(eng, 21 + step, scale=0.05)
            eng.fold()
            grads = named_grads(net)
            active = [n for li, mod in eng.active_slots() for n in PR.names(PR.layers(start)[0][li], mod)]
            if ref_opt is None:
                ref_opt = torch.optim.SGD([cpu[n] for n in active], lr=G.LR, momentum=G.MOMENTUM, weight_decay=G.WD)
            for n in active:
                cpu[n].grad = grads[n].clone()
            norm = float(torch.nn.utils.clip_grad_norm_([cpu[n] for n in active], clip))
            assert (norm > clip) == (clip < 100), (norm, clip)   # the case does what it says
            ref_opt.step()
            eng.sgd(opt, clip)
            torch.cuda.synchronize()
            now = own_state(net)
            for n in active:
                assert PR.rel(now[n], cpu[n].detach()) <= 1e-6, (step, n)
                assert PR.rel(net.get_parameter(n).grad, cpu[n].grad) <= 1e-6, (step, n)
            for n in now:
                if n not in active:
                    assert torch.equal(now[n], start[n]), n      # frozen slots: bitwise
            seen.append(torch.cat([v.reshape(-1) for v in now.values()]))
        buf = opt.buf.cpu()
        assert int(torch.isnan(buf).sum()) == buf.numel() - sum(start[n].numel() for n in active)
        runs.append(seen)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_engine_step_matches_g38(golden, case):
    """Net.forward logits, CE and the parameters after one train_epoch (batches 40, 40, 7) against the reference's record,
    at the tolerances of the HAT step test (pathnet_ref.assert_matches_g38); what G38 did not move stays bitwise."""
    from clsurvey_amd.methods import pathnet as PN
    g = golden("G38_pathnet_step")
    c = G.CASES[case]
    net, eng, start = build(c["setting"], c["best0"])
    eng.set_path(np.array(c["path"]), c["t"])
    data = [(torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())) for x, y in G.batches(case)]
    net.eval()
    logits = eng.forward(data[0][0]).cpu()
    loss = eng.loss(data[0][0], data[0][1])[0].cpu().clone()
    net.train()
    opt = PN.PathSGD(eng, G.LR, G.MOMENTUM, G.WD)
    for x, y in data:
        eng.step(x, y, opt, c["clipgrad"])
    torch.cuda.synchronize()
    PR.assert_matches_g38(g, case, logits, loss, own_state(net), start)
    snap = eng.snapshot()
    eng.step(data[0][0], data[0][1], opt, c["clipgrad"])
    eng.restore(snap)
    assert torch.equal(eng.A.theta, snap)


def test_dropout_models_draw_a_mask_over_every_packed_input():
    """*_DROP models: drop_fc(relu(fc_m(x))) per module (vgg_pathnet.py:119-124) is one mask over the N*f inputs of the next
    packed layer; identity in eval mode."""
    import torch.nn as nn
    from clsurvey_amd import models
    from clsurvey_amd.methods import pathnet as PN
    raw = models.VGGSlim(cfg=G.CFG, num_classes=G.NCLS, classifier_inputdim=64 * 2 * 2, classifier_dim1=G.FC[0],
                         classifier_dim2=G.FC[1])
    fc = [m for m in raw.classifier.children() if isinstance(m, nn.Linear)]
    raw.classifier = nn.Sequential(fc[0], nn.ReLU(True), nn.Dropout(0.5), fc[1], nn.ReLU(True), nn.Dropout(0.5), fc[2])
    net = PN.PathNet(raw, (3, G.HW, G.HW), [(t, G.NCLS) for t in range(G.NTASKS)], [2, 4])
    assert net.drop_p == 0.5
    eng = PN.PathEngine(net, 40, (3, G.HW, G.HW), dev())
    assert sorted(eng.engine.drops) == [7, 8]                      # in front of the second Linear layer and of the head
    path = np.array(G.A_PLAIN)
    eng.set_path(path, 0)
    x, y = (torch.from_numpy(v).to(dev()) for v in G.batches("a_plain")[0])
    net.eval()
    a, b = eng.forward(x).clone(), eng.forward(x).clone()
    assert torch.equal(a, b)
    with torch.no_grad():
        want = PR.direct_forward(own_state(net), x.cpu(), path, 2, MAXPOOL)
    assert PR.rel(a, want) <= PR.TOL_LOGITS
    net.train()
    c, d = eng.forward(x).clone(), eng.forward(x).clone()
    assert not torch.equal(c, d) and not torch.equal(c, a)
    before = own_state(net)
    eng.step(x, y, PN.PathSGD(eng, G.LR, G.MOMENTUM, G.WD), 1000.0)
    after = own_state(net)
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert not torch.equal(after["fcs.1.%d.weight" % path[7][0]], before["fcs.1.%d.weight" % path[7][0]])
    net.eval()
    assert not torch.equal(eng.forward(x), a)                      # the evaluation after a step packs the moved modules
