"""LwF and EBLL with heads of any size and sequences of up to 64 tasks, on the TINY net of test_gpu_parity._g14_wrapper
(3 x 32 x 32 input, VGGSlim(cfg=TINY), batch 8): the packed head runs of the parameter arena under the plan executor, the
choice between clhip_lwf_loss and clhip_lwf_loss_wide, LwfEngine.step / EbllEngine.step against oracle.vgg_ref +
oracle.lwf_ref / oracle.ebll_ref evaluated with torch on the CPU in fp32 (bounds of the G14 / G16 tests: 2e-4 logits, 1e-4
losses, 1e-3 gradients, each relative to the tensor's largest entry), and the LwF trainers on three tasks of 5, 3 and 6 classes.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ebll_ref, lwf_ref, vgg_ref

pytestmark = pytest.mark.gpu

TINY = [16, "M", 16, "M", 32, 32, "M", 32, 32, "M"]
N = 8


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def assert_close(a, b, tol, what):
    e = rel_err(a, b)
    assert e <= tol, "%s rel err %.3e > %.1e" % (what, e, tol)


def _pad4(n):
    return (n + 3) // 4 * 4


def _net(sizes, seed):
    """(VGGSlim with the first head, [(weight, bias)] of all heads, the oracle's flat parameter list of the shared layers)."""
    from clsurvey_amd import models
    gen = np.random.RandomState(seed)
    ps = vgg_ref.init_params(TINY, (24, 24), sizes[0], 32, gen)
    for i in (-6, -4, -2):                                   # as _g14_wrapper: logits of a useful size
        ps[i] = ps[i] * 20.0
    m = models.VGGSlim(cfg=TINY, num_classes=sizes[0], classifier_inputdim=32 * 2 * 2, classifier_dim1=24, classifier_dim2=24)
    with torch.no_grad():
        for p, q in zip(m.parameters(), ps):
            p.copy_(q)
    heads = [(ps[-2], ps[-1])]
    for nc in sizes[1:]:
        heads.append((torch.from_numpy((gen.standard_normal((nc, 24)) * 0.2).astype(np.float32)),
                      torch.from_numpy((gen.standard_normal((nc,)) * 0.01).astype(np.float32))))
    return m, heads, ps[:-2]


def _add_heads(classifier, heads):
    for i, (hw_, hb) in enumerate(heads[1:]):
        h = torch.nn.Linear(24, hw_.shape[0])
        with torch.no_grad():
            h.weight.copy_(hw_)
            h.bias.copy_(hb)
        classifier.add_module(str(5 + i), h)


def _lwf_wrapper(sizes, seed):
    from clsurvey_amd.methods import lwf as LF
    m, heads, shared = _net(sizes, seed)
    w = LF.AlexNet_LwF(m, last_layer_name=4)
    _add_heads(w.model.classifier, heads)
    return w, heads, shared


def _batch(sizes, seed):
    gen = np.random.RandomState(seed)
    x = torch.from_numpy(gen.standard_normal((N, 3, 32, 32)).astype(np.float32))
    y = torch.from_numpy(gen.randint(0, sizes[-1], size=(N,)).astype(np.int64))
    teacher = torch.from_numpy((gen.standard_normal((N, sum(sizes[:-1]))) * 2).astype(np.float32))
    return x, y, teacher


def _lwf_oracle(shared, heads, x, y, teacher, T, lam):
    """torch CPU fp32: (head outputs, task, lambda * distillation, gradients of [shared..., head weights..., head biases...])."""
    leaves = [p.detach().clone().requires_grad_(True) for p in list(shared) + [h[0] for h in heads] + [h[1] for h in heads]]
    ns, nh = len(shared), len(heads)
    h = F.relu(vgg_ref.forward(leaves[:ns], TINY, x))         # forward leaves the last Linear bare: the heads' input has a ReLU
    outs = [F.linear(h, leaves[ns + i], leaves[ns + nh + i]) for i in range(nh)]
    offs = np.cumsum([0] + [o.shape[1] for o in outs[:-1]])
    tt = [teacher[:, offs[i]:offs[i + 1]] for i in range(nh - 1)]
    task, dist = lwf_ref.lwf_objective(outs, y, tt, T, lam)
    grads = torch.autograd.grad(task + dist, leaves)
    return [o.detach() for o in outs], task.detach(), dist.detach(), grads


def _engine_params(w):
    """The arena order of lwf_plan: shared layers, head weights, head biases."""
    cls = list(w.model.classifier.children())
    heads = cls[w.last_layer_name:]
    shared = list(w.model.features.parameters()) + [p for m in cls[:w.last_layer_name] for p in m.parameters()]
    return shared + [h.weight for h in heads] + [h.bias for h in heads]


def _step_against_oracle(sizes, seed, T=2.0, lam=10.0):
    from clsurvey_amd.methods import lwf as LF
    w, heads, shared = _lwf_wrapper(sizes, seed)
    x, y, teacher = _batch(sizes, seed + 1)
    outs, task, dist, grads = _lwf_oracle(shared, heads, x, y, teacher, T, lam)
    d = dev()
    w = w.to(d)
    eng = LF.LwfEngine(w, N, (3, 32, 32), d)
    assert eng.sizes == list(sizes)
    xd, yd, td = x.to(d), y.to(d), teacher.to(d)
    z = eng.logits(xd)
    assert_close(z, torch.cat(outs, 1), 2e-4, "stacked logits")
    stats = torch.zeros(2, dtype=torch.float64, device=d)
    loss2 = eng.step(xd, yd, td, T, lam, backward=True, stats=stats).clone()
    assert_close(loss2[0:1], task.view(1), 1e-4, "task loss")
    assert_close(loss2[1:2], dist.view(1), 1e-4, "lambda * distillation")
    assert int(stats[1].item()) == int((outs[-1].argmax(1) == y).sum())
    params = _engine_params(w)
    assert len(params) == len(grads)
    got = [p.grad.clone() for p in params]
    for j, (g_dev, g_ref) in enumerate(zip(got, grads)):
        assert_close(g_dev, g_ref, 1e-3, "grad %d of %d %s" % (j, len(grads), tuple(g_ref.shape)))
    return w, eng, (xd, yd, td), outs, got


def test_odd_heads_step_matches_the_oracle():
    sizes = [5, 3, 6]
    w, eng, (xd, yd, td), outs, got = _step_against_oracle(sizes, 301)
    assert eng.wide is True
    a = eng.arena
    nh = len(sizes)
    wo, bo = a.offsets[-2 * nh], a.offsets[-nh]
    assert wo % 4 == 0 and bo % 4 == 0
    assert a.offsets[-2 * nh:-nh] == [wo, wo + 5 * 24, wo + 8 * 24] and a.offsets[-nh:] == [bo, bo + 5, bo + 8]
    # the wrapper's bridge forward (the evaluation path) reads the heads at their 4-byte aligned places in the arena
    with torch.no_grad():
        bridge = w(xd)
    z = eng.logits(xd)
    off = 0
    for i, (o, ref) in enumerate(zip(bridge, outs)):
        assert_close(o, ref, 2e-4, "bridge head %d" % i)
        assert_close(z[:, off:off + sizes[i]], o, 2e-4, "stacked logits vs bridge, head %d" % i)
        off += sizes[i]
    # a second identical step from the same state: bitwise the same gradients
    eng.step(xd, yd, td, 2.0, 10.0, backward=True)
    for j, (p, g) in enumerate(zip(_engine_params(w), got)):
        assert torch.equal(p.grad, g), "gradient %d differs between two identical steps" % j
    # validation: no teacher, no backward
    stats = torch.zeros(2, dtype=torch.float64, device=dev())
    loss2 = eng.step(xd, yd, None, 2.0, 10.0, backward=False, stats=stats)
    assert float(loss2[1]) == 0.0 and float(stats[0]) == float(loss2[0])


def test_multiple_of_4_heads_keep_the_kernel_and_the_arena():
    from clsurvey_amd.methods import lwf as LF
    w, heads, shared = _lwf_wrapper([8, 4, 4], 302)
    d = dev()
    w = w.to(d)
    eng = LF.LwfEngine(w, N, (3, 32, 32), d)
    assert eng.wide is False and eng.arena.runs is None
    off, want = 0, []
    for p in eng.arena.params:
        want.append(off)
        off += _pad4(p.numel())
    assert eng.arena.offsets == want and eng.arena.numel == off
    # both kernels can be forced on this plan; the default is the narrow one
    assert LF.LwfEngine(copy.deepcopy(w), N, (3, 32, 32), d, wide=True).wide is True
    w33, _, _ = _lwf_wrapper([4] * 33, 303)
    with pytest.raises(NotImplementedError):
        LF.LwfEngine(w33.to(d), N, (3, 32, 32), d, wide=False)


@pytest.mark.parametrize("layout", ["40x5", "63x3+4"])
def test_long_sequences_step_matches_the_oracle(layout):
    sizes = {"40x5": [5] * 40, "63x3+4": [3] * 63 + [4]}[layout]
    w, eng, _, _, _ = _step_against_oracle(sizes, 310 + len(sizes))
    assert eng.wide is True and len(eng.sizes) == len(sizes)


def test_ebll_step_odd_heads_matches_the_oracle():
    """EbllEngine.step with heads [5, 3] and one encoder of code width 10, with the structure and the bounds of
    test_ebll_objective_golden_g16; the reference is oracle.ebll_ref.stage2_objective on torch CPU."""
    from clsurvey_amd.methods import ebll as E
    sizes = [5, 3]
    m, heads, shared = _net(sizes, 320)
    gen = np.random.RandomState(321)
    ae = E.AutoEncoder(128, 10)
    we = torch.from_numpy((gen.standard_normal((10, 128)) * 0.3).astype(np.float32))
    be = torch.from_numpy((gen.standard_normal((10,)) * 0.05).astype(np.float32))
    with torch.no_grad():
        ae.encode[0].weight.copy_(we)
        ae.encode[0].bias.copy_(be)
    w = E.AlexNet_EBLL(m, ae, last_layer_name=4)
    _add_heads(w.classifier, heads)
    x, y, tl = _batch(sizes, 322)
    tcode = torch.from_numpy(gen.uniform(0.1, 0.9, (N, 10)).astype(np.float32))
    T, lam, alpha = 2.0, 3.0, 2.0
    # ---- torch CPU fp32
    leaves = [p.detach().clone().requires_grad_(True) for p in list(shared) + [h[0] for h in heads] + [h[1] for h in heads]]
    ns, nconv = len(shared), 2 * vgg_ref.n_conv(TINY)
    feat = torch.flatten(vgg_ref.features(leaves[:nconv], TINY, x), 1)
    code = ebll_ref.encode(feat, we, be)
    h = F.relu(F.linear(F.relu(F.linear(feat, leaves[nconv], leaves[nconv + 1])), leaves[nconv + 2], leaves[nconv + 3]))
    outs = [F.linear(h, leaves[ns + i], leaves[ns + 2 + i]) for i in range(2)]
    task, dist, closs = ebll_ref.stage2_objective(outs, [code], y, [tl], [tcode], T, lam, alpha)
    grads = torch.autograd.grad(task + dist + alpha * closs, leaves)
    task, dist, closs = float(task.detach()), float(dist.detach()), float(closs.detach())
    # ---- device
    d = dev()
    w = w.to(d)
    xd = x.to(d)
    with torch.no_grad():
        bridge_outs, bridge_codes = w(xd)                    # evaluation path of the wrapper
    for i in range(2):
        assert_close(bridge_outs[i], outs[i].detach(), 1e-4, "out%d" % i)
    assert_close(bridge_codes[0], code.detach(), 1e-5, "code0")
    eng = E.EbllEngine(w, N, (3, 32, 32), d)
    assert eng.lwf.wide is True and eng.lwf.sizes == sizes
    loss2, code_loss = eng.step(xd, y.to(d), tl.to(d), [tcode.to(d)], T, lam, alpha, backward=True)
    assert abs(float(loss2[0]) - task) <= 1e-4 * abs(task)
    assert abs(float(loss2[1]) - dist) <= 1e-4 * abs(dist)
    assert abs(float(code_loss) - closs) <= 1e-4 * abs(closs)
    cls = list(w.classifier.children())
    params = list(w.features.parameters()) + [p for mod in cls[:4] for p in mod.parameters()] + \
        [mod.weight for mod in cls[4:]] + [mod.bias for mod in cls[4:]]
    assert len(params) == len(grads)
    for j, (p, g) in enumerate(zip(params, grads)):
        assert_close(eng.arena.view("grad", p), g, 1e-3, "grad %d %s" % (j, tuple(g.shape)))
    t_logits, t_codes = eng.targets(xd)                      # targets() of a teacher engine = the wrapper's own outputs / codes
    assert_close(t_logits, torch.cat([o.detach() for o in outs], 1), 1e-4, "targets")
    assert_close(t_codes[0], code.detach(), 1e-5, "target codes")


def test_lwf_trainers_on_tasks_of_5_3_and_6_classes(tmp_path):
    """Task 1 by fine_tune_SGD, tasks 2 and 3 by fine_tune_SGD_LwF (no head warm-up): the run completes, the saved wrapper
    holds heads of 5, 3 and 6 classes and its engine and its bridge forward agree."""
    from clsurvey_amd import data, models
    from clsurvey_amd.methods import finetune, lwf
    from clsurvey_amd.methods.method import compose_dataset
    d = "cuda:0"
    root = str(tmp_path)
    classes = [5, 3, 6]
    paths = []
    for t, n in enumerate(classes):
        paths.append(os.path.join(root, "task%d.pth.tar" % t))
        torch.save(data.synthetic_task(40, 20, 20, n, hw=32), paths[-1])
    torch.manual_seed(0)
    m = models.VGGSlim(cfg=TINY, num_classes=classes[0], classifier_inputdim=32 * 2 * 2, classifier_dim1=24, classifier_dim2=24)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    base = os.path.join(root, "base.pth.tar")
    torch.save(m, base)
    loaders, sizes, cls = compose_dataset([paths[0]], 20, d)
    _, acc = finetune.fine_tune_SGD(loaders, sizes, cls, base, os.path.join(root, "t0"), num_epochs=2, lr=1e-2, device=d,
                                    batch_size=20)
    assert 0.0 <= acc <= 1.0
    prev = os.path.join(root, "t0", "best_model.pth.tar")
    for t in (1, 2):
        exp = os.path.join(root, "t%d" % t)
        model, acc = lwf.fine_tune_SGD_LwF(paths[t], prev, exp_dir=exp, batch_size=20, num_epochs=2, lr=1e-2, init_freeze=0,
                                           last_layer_name=4, device=d)
        assert np.isfinite(acc) and 0.0 <= acc <= 1.0
        prev = os.path.join(exp, "best_model.pth.tar")
        assert os.path.isfile(prev) and os.path.isfile(os.path.join(exp, "epoch.pth.tar"))
    saved = torch.load(prev, weights_only=False)
    assert isinstance(saved, lwf.AlexNet_LwF) and saved.last_layer_name == 4
    assert [h.out_features for h in list(saved.model.classifier.children())[4:]] == classes
    saved = saved.to(d).eval()
    eng = lwf.LwfEngine(saved, 20, (3, 32, 32), d)
    assert eng.wide is True and eng.sizes == classes
    x = torch.randn(20, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(d)
    with torch.no_grad():
        bridge = saved(x)
    assert all(bool(torch.isfinite(o).all()) for o in bridge)
    assert_close(eng.logits(x), torch.cat(bridge, 1), 2e-4, "engine logits vs bridge forward of the saved model")
