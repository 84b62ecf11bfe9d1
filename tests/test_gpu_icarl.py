"""iCaRL on the MI355X: herding against fixture G37 (tests/golden/make_g37.py) and against a torch restatement at a
realistic size, the CE + distillation loss and the nearest-mean classifier against torch, a replay of G37's task-3 steps
(fused and segmented) with the recorded dropout masks, and one run through the driver."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g37_common as I  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _fixture():
    with open(os.path.join(HERE, "golden", "G37_icarl.json")) as f:
        return json.load(f), np.load(os.path.join(HERE, "golden", "G37_icarl.npz"))


# --------------------------------------------------------------------------- herding
def test_herding_matches_g37_rankings():
    """Every class of every manage_memory of the fixture, all picks (the generator asserted a relative gap >= 1e-4 between
    the best and the second-best cost at every pick): the rankings are equal."""
    from clsurvey_amd import ops
    meta, npz = _fixture()
    for t, rec in enumerate(meta["manage"]):
        feats = [npz["m%d_c%d_feats" % (t, c)] for c in range(4)]
        w = np.concatenate([npz["m%d_c%d_w" % (t, c)] for c in range(4)])
        bounds = np.concatenate([[0], np.cumsum([len(f) for f in feats])])
        ks = [len(c["ranking"]) for c in rec["classes"]]
        got = ops.icarl_herd(torch.from_numpy(np.concatenate(feats)).to(DEV), torch.from_numpy(w).to(DEV),
                             [(int(bounds[c]), int(bounds[c + 1])) for c in range(4)], ks)
        for c in range(4):
            assert got[c].cpu().tolist() == rec["classes"][c]["ranking"], (t, c)


def _herd_restatement(f, w, K):
    """icarl.py:397-457 on features computed once (float32 torch on the host), with the smallest relative gap seen."""
    mu = (f.double() * w.double()[:, None]).sum(0).float()
    taken = torch.zeros(len(f), dtype=torch.bool)
    prev = torch.zeros(f.shape[1])
    rank, worst = [], float("inf")
    for k in range(K):
        cost = (mu.unsqueeze(0) - (f + prev.unsqueeze(0)) / (k + 1)).norm(2, 1).double()
        cost[taken] = float("inf")
        best2 = torch.topk(cost, 2, largest=False)
        win = int(best2.indices[0])
        if torch.isfinite(best2.values[1]):
            worst = min(worst, float((best2.values[1] - best2.values[0]) / best2.values[0]))
        taken[win] = True
        rank.append(win)
        prev = prev + f[win]
    return rank, worst


def test_herding_matches_torch_at_realistic_size():
    """A class of 400 rows, F = 2048, K = 100 (and a second, shorter class with an odd row count in the same launch); the
    gap condition (>= 1e-4 relative at every pick) is checked on the restatement first.  The features are a ReLU of a rank-3
    pattern plus noise: independent coordinates would put all 400 distances within ~1/sqrt(F) of each other and no seed keeps
    a 1e-4 gap over 100 picks."""
    from clsurvey_amd import ops
    from clsurvey_amd.methods.icarl import mean_weights
    gen = torch.Generator().manual_seed(38)
    sizes, ks = [400, 137], [100, 40]
    n = sum(sizes)
    f = torch.relu(torch.randn((n, 3), generator=gen) @ torch.randn((3, 2048), generator=gen) + 0.05 * torch.randn((n, 2048), generator=gen))
    w = torch.from_numpy(np.concatenate([mean_weights(n, 132) for n in sizes]))
    want, lo = [], 0
    for n, k in zip(sizes, ks):
        rank, gap = _herd_restatement(f[lo:lo + n], w[lo:lo + n], k)
        assert gap >= 1e-4, "restatement gap %.3g: change the seed of this test's data" % gap
        want.append(rank)
        lo += n
    got = ops.icarl_herd(f.to(DEV), w.to(DEV), [(0, 400), (400, 537)], ks)
    assert [g.cpu().tolist() for g in got] == want


# --------------------------------------------------------------------------- loss
def _loss_restatement(z, y, tg, segs, T=2.0):
    z = z.clone().double().requires_grad_(True)
    total = torch.zeros((), dtype=torch.float64)
    for r0, r1, o, nc, sc, kind in segs:
        zs = z[r0:r1, o:o + nc]
        if kind == 0:
            v = torch.nn.functional.cross_entropy(zs, y[r0:r1])
        else:
            v = torch.nn.KLDivLoss(reduction="batchmean")(torch.log_softmax(zs / T, 1), torch.softmax(tg[r0:r1, o:o + nc].double() / T, 1)) * T ** 2
            if float(v) < 0:
                v = v * 0
        total = total + sc * v
    total.backward()
    return float(total), z.grad


def test_loss_segments_match_torch():
    """Value and gradient against float64 torch: CE on the last slice of the head, distillation on the first and on a middle
    slice, two chunks of one task, unequal scales.  Bounds from the number format: a row's KL sums p (log p - log q) with both
    logarithms of magnitude <= ~8 rounded in fp32 (2^-24 * 8 = 5e-7 each), times T^2 = 4: <= 4e-6 absolute per row in the worst
    case on a loss of O(1..10) => 5e-6 relative on the value; a gradient entry is T * scale / rows * (q - p) with q, p in [0, 1]
    at fp32 exp accuracy => 1e-6 absolute (the bound test_gpu_rehearsal.py uses for the CE gradient)."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(3)
    N, ld = 23, 12
    z = torch.randn((N, ld), generator=gen) * 2
    tg = torch.randn((N, ld), generator=gen) * 2
    y = torch.randint(0, 4, (N,), generator=gen)
    segs = [(0, 9, 8, 4, 1.0, 0), (9, 14, 0, 4, 2.75, 1), (14, 16, 0, 4, 2.75, 1), (16, 23, 4, 4, 0.5, 1)]
    want, gwant = _loss_restatement(z, y, tg, segs)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    loss, dz = ops.loss_segments(z.to(DEV), y.to(DEV), tg.to(DEV), ops.loss_segment_table(segs, DEV), len(segs), 2.0, stats)
    assert abs(float(loss) - want) <= 5e-6 * abs(want)
    assert float((dz.double().cpu() - gwant).abs().max()) <= 1e-6
    hits = int((z[:9, 8:12].argmax(1) == y[:9]).sum())
    assert int(stats[1]) == hits and abs(float(stats[0]) - float(loss)) < 1e-12


def test_loss_segment_with_target_equal_to_logits_adds_nothing():
    """KL of a distribution with itself is 0 up to rounding and may come out negative, which the reference replaces by the
    integer 0 (:584-587): such a segment adds nothing and its rows get zero gradient."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(4)
    z = torch.randn((10, 12), generator=gen) * 3
    y = torch.randint(0, 4, (10,), generator=gen)
    segs = [(0, 4, 0, 4, 1.0, 0), (4, 10, 4, 4, 7.0, 1)]
    only_ce, _ = _loss_restatement(z, y, z, segs[:1])
    loss, dz = ops.loss_segments(z.to(DEV), y.to(DEV), z.clone().to(DEV), ops.loss_segment_table(segs, DEV), 2)
    assert abs(float(loss) - only_ce) <= 1e-6 * abs(only_ce)
    assert float(dz[4:].abs().max()) <= 1e-7 and float(dz[:4].abs().max()) > 0


def test_negative_distillation_chunk_is_gated_on_the_device():
    """Targets a hair away from the logits: the true KL is ~1e-9 while the fp32 value carries ~1e-7 of rounding of either
    sign, so about half of such chunks come out negative before the gate (:584-587) while softmax(z/T) != softmax(target/T).
    64 candidates, one launch each (one distillation segment of scale 1): the loss is never negative; a chunk reported as
    exactly 0 has an all-zero gradient although the float64 gradient of its KL is not zero (the gate took it: at least one
    candidate must be such a chunk, or this test does not reach the branch and fails); every other chunk has a gradient."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(6)
    seg = ops.loss_segment_table([(0, 5, 4, 4, 1.0, 1)], DEV)
    y = torch.zeros(5, dtype=torch.int64, device=DEV)
    gated = 0
    for _ in range(64):
        z = torch.randn((5, 12), generator=gen) * 3
        tg = z + 1e-4 * torch.randn((5, 12), generator=gen)
        _, g64 = _loss_restatement(z, None, tg, [(0, 5, 4, 4, 1.0, 1)])
        assert float(g64.abs().max()) > 1e-7                       # q != p
        loss, dz = ops.loss_segments(z.to(DEV), y, tg.to(DEV), seg, 1)
        v = float(loss)
        assert v >= 0.0 and v < 1e-5
        if v == 0.0:
            assert float(dz.abs().max()) == 0.0
            gated += 1
        else:
            assert float(dz[:, 4:8].abs().max()) > 0 and float(dz[:, :4].abs().max()) == 0 and float(dz[:, 8:].abs().max()) == 0
    assert gated >= 1, "no candidate was negative before the gate"


def test_loss_malformed_segment_is_nan():
    from clsurvey_amd import ops
    z = torch.randn((6, 12), device=DEV)
    y = torch.zeros(6, dtype=torch.int64, device=DEV)
    for bad in ((0, 7, 0, 4, 1.0, 0), (0, 6, 10, 4, 1.0, 1), (0, 6, 0, 4, 1.0, 2), (3, 3, 0, 4, 1.0, 0)):
        loss, _ = ops.loss_segments(z, y, z.clone(), ops.loss_segment_table([bad], DEV), 1)
        assert bool(torch.isnan(loss).all()), bad
    loss, _ = ops.loss_segments(z, y, None, ops.loss_segment_table([(0, 6, 0, 4, 1.0, 1)], DEV), 1)      # distillation without targets
    assert bool(torch.isnan(loss).all())


# --------------------------------------------------------------------------- nearest mean
def test_nme_matches_torch_with_ties():
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(5)
    N, F, C, o1, n_out = 37, 256, 5, 4, 12
    means = torch.randn((C, F), generator=gen)
    means[3] = means[1]                                   # an exact tie: the first minimum wins
    x = means[torch.randint(0, C, (N,), generator=gen)] + 0.3 * torch.randn((N, F), generator=gen)
    dist = (means.unsqueeze(0) - x.unsqueeze(1)).norm(2, 2)
    srt = dist.sort(1).values
    assert float(((srt[:, 1] - srt[:, 0])[dist.argmin(1) != 1]).min()) > 1e-3        # no near-ties besides the planted one
    want = torch.zeros(N, n_out)
    arg = torch.tensor([int(d.min(0)[1]) for d in dist])
    arg[arg == 3] = 1
    want[torch.arange(N), o1 + arg] = 1
    got = ops.icarl_nme(x.to(DEV), means.to(DEV), o1, C, n_out)
    assert torch.equal(got.cpu(), want) and int((arg == 1).sum()) > 0
    empty = ops.icarl_nme(None, None, o1, C, n_out, n_rows=3).cpu()
    assert bool((empty[:, o1:o1 + C] == 1.0 / C).all()) and bool((empty[:, :o1] == -10e10).all()) and bool((empty[:, o1 + C:] == -10e10).all())


# --------------------------------------------------------------------------- fixture replay
def _wrapper(npz, tag):
    from clsurvey_amd.methods.icarl import IcarlNet
    net = I.make_net()
    w = IcarlNet(net, I.N_OUT, I.N_TASKS, I.NC_PER_TASK, I.N_MEMORIES, I.LR, I.WD, I.REG, I.B + I.N_APPEND, (3, I.HW, I.HW), "cuda")
    _load(w, npz, tag)
    return w


def _load(w, npz, tag):
    with torch.no_grad():
        for i, p in enumerate(w.net.parameters()):
            p.copy_(torch.from_numpy(npz["%s_%d" % (tag, i)]))


def _postprocess(w, t):
    import types
    from clsurvey_amd.data import TensorTaskDataset
    x, y = I.task_data(t)
    args = types.SimpleNamespace(task_imgfolders={"train": TensorTaskDataset(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), [])},
                                 batch_size=I.HERD_BATCH)
    w.manage_memory(t, args)


def _check_store(w, meta, npz, t):
    rec = meta["manage"][t]
    assert w.exemplar_count == rec["exemplar_count"]
    assert {str(c): n for c, n in enumerate(w.class_len)} == rec["lengths"]
    ranking, offs = w.last_ranking
    assert [ranking[int(offs[c]):int(offs[c + 1])].cpu().tolist() for c in range(4)] == [c["ranking"] for c in rec["classes"]]
    for task in range(t + 1):                       # stored rows and distillation targets, truncated blocks included
        x, _ = I.task_data(task)
        for c in range(4):
            cls = 4 * task + c
            r0, n = w._block(cls)
            cr = meta["manage"][task]["classes"][c]
            rows = [cr["rows"][i] for i in cr["ranking"][:n]]
            assert torch.equal(w.store_x[r0:r0 + n].cpu(), torch.from_numpy(x[rows])), (t, cls)
            ref_y = torch.from_numpy(npz["m%d_c%d_y" % (task, c)][:n])
            got_y = w.store_t[r0:r0 + n].cpu()
            assert torch.equal(got_y < -1e10, ref_y < -1e10)
            inside = ref_y > -1e10
            assert float((got_y[inside] - ref_y[inside]).abs().max()) <= 1e-4 * float(ref_y[inside].abs().max()), (t, cls)


def _nme_check(w, npz, m):
    import types
    probe = torch.from_numpy(I.probe_batch()).to(DEV)
    for task in range(I.N_TASKS):
        out = w(probe, task, args=types.SimpleNamespace(batch_size=I.EVAL_BATCH))
        assert torch.equal(out.cpu(), torch.from_numpy(npz["nme_m%d_t%d" % (m, task)])), (m, task)


def _replay(force_segmented):
    meta, npz = _fixture()
    w = _wrapper(npz, "p_init")
    _postprocess(w, 0)
    _check_store(w, meta, npz, 0)
    _nme_check(w, npz, 0)
    _load(w, npz, "p_task2")
    w._means = {}
    _postprocess(w, 1)
    _check_store(w, meta, npz, 1)
    _nme_check(w, npz, 1)
    w.init_setup(lr=I.LR, weight_decay=I.WD, memory_strength=I.REG, n_append=I.N_APPEND, chunk_size=I.HERD_BATCH,
                 total_batch_size=I.TOTAL_BATCH)
    w.force_segmented = force_segmented
    I.seed_draws(2)
    lis = sorted(w.engine.drops)
    losses, grads = [], None
    for k, ((x, y), rec) in enumerate(zip(I.step_batches(2, I.STEPS), meta["steps"])):
        masks = {li: torch.from_numpy(npz["s%d_mask%d" % (k, d)]).to(DEV).contiguous() for d, li in enumerate(lis)}
        w._draw_mask = lambda li, n, elems, p, _m=masks: _m[li][:n].contiguous()
        loss, hits, _ = w.observe(torch.from_numpy(x).to(DEV), 2, torch.from_numpy(y).to(DEV))
        assert w.last_path == ("segmented" if force_segmented else "fused")
        assert int(hits) == rec["hits"], k
        losses.append(float(loss))
        if k == 0:
            grads = w.A.grad.clone()
            got = [w.A.grad[w.A.slot(p)[0]:w.A.slot(p)[0] + p.numel()].view_as(p).cpu() for p in w.net.parameters()]
            for i, g in enumerate(got):
                ref = torch.from_numpy(npz["s0_grad_%d" % i])
                err = float((g.double() - ref.double()).abs().max())
                assert err <= 1e-3 * max(float(ref.abs().max()), 1e-6), (i, err)
    for k, rec in enumerate(meta["steps"]):
        assert abs(losses[k] - rec["loss"]) <= 3e-4 * abs(rec["loss"]), (k, losses[k], rec["loss"])
    for i, p in enumerate(w.net.parameters()):
        ref = torch.from_numpy(npz["p_task3_%d" % i])
        err = float((p.data.double().cpu() - ref.double()).abs().max())
        assert err <= 1e-3 * max(float(ref.abs().max()), 1e-6), (i, err)
    return w, losses, grads, meta, npz


def test_g37_replay_fused_and_segmented():
    """G37: manage_memory at tasks 1-2 (rankings, stored rows, distillation targets, nearest-mean outputs), then the task-3
    steps with the recorded masks on both paths.  Bounds as test_gpu_rehearsal.py::test_g35_replay: losses within 3e-4,
    hits exact, first-step gradients and final parameters rel_err <= 1e-3 against the fixture; fused against segmented:
    loss 1e-5, gradient 1e-3 (test_fused_step_matches_segmented_step_task10)."""
    wf, lf, gf, meta, npz = _replay(False)
    ws, ls, gs, _, _ = _replay(True)
    for a, b in zip(lf, ls):
        assert abs(a - b) <= 1e-5 * abs(b)
    assert rel_err(gf, gs) <= 1e-3
    # the third manage_memory (K/m = 2: every stored class truncated again) on the fixture's own parameters, and a reload
    _load(wf, npz, "p_task3")
    wf._means = {}
    _postprocess(wf, 2)
    _check_store(wf, meta, npz, 2)
    _nme_check(wf, npz, 2)
    buf = io.BytesIO()
    torch.save(wf, buf)
    buf.seek(0)
    w2 = torch.load(buf, weights_only=False)
    assert w2.class_len == [2] * 12 and torch.equal(w2.store_x, wf.store_x) and torch.equal(w2.store_t, wf.store_t)
    assert wf.__getstate__()["_rows_x"].shape[0] == 24
    _nme_check(w2, npz, 2)


def test_manage_memory_refuses_batchnorm_features():
    import g35_common as I35
    from clsurvey_amd.methods.icarl import IcarlNet
    w = IcarlNet(I35.make_net(True), I.N_OUT, I.N_TASKS, I.NC_PER_TASK, I.N_MEMORIES, I.LR, I.WD, I.REG, 8, (3, I.HW, I.HW), "cuda")
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        _postprocess(w, 0)


# --------------------------------------------------------------------------- driver
def _storage_sizes(path):
    import zipfile
    with zipfile.ZipFile(path) as z:
        return sorted(i.file_size for i in z.infolist() if "/data/" in i.filename and not i.filename.endswith(".pkl"))


def test_icarl_through_driver(tmp_path):
    """An SI first-task dump, then 3 tasks of ICARL with --test on a synthetic sequence: task 1 wraps the SI model with its
    herded exemplars, tasks 2-3 train (phase-1 observe_FT grid, phase-2 observe with distillation) and are postprocessed; the
    wrappers reload, the per-class exemplar counts follow K/m, the pickles hold the stored rows only, accuracies (nearest
    mean of exemplars) are finite and above chance."""
    from clsurvey_amd import models
    from clsurvey_amd.framework import driver
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import method as M
    root = str(tmp_path)
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=3, classes_per_task=4, sizes=(160, 40, 40), hw=32,
                               noise=0.4, name="tiny3")
    torch.manual_seed(0)
    base = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in base.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(base, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))
    common = ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "6", "--batch_size", "40", "--saving_freq", "100"]
    driver.main(common + ["--method_name", "SI", "--results_root", root, "--runmode", "first_task_basemodel_dump"],
                method=M.parse("SI"), dataset=ds)
    icarl = M.parse("ICARL")
    K = 16
    icarl.static_hyperparams = {"mem_per_task": K}
    out = driver.main(common + ["--method_name", "ICARL", "--results_root", root, "--test"], method=icarl, dataset=ds)
    res = out["results"]
    assert sorted(res) == [0, 1, 2]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    assert all(np.isfinite(a) and 0.0 <= a <= 100.0 for a in accs)
    assert all(res[i]["seq_res"][i][0] > 35.0 for i in res), res              # chance is 25 %
    paths = out["model_paths"]
    assert len(paths) == 3 and paths[0].endswith("best_model.pth.tar")
    assert all(p.endswith("best_model_postprocessed.pth.tar") for p in paths[1:])
    total, row_bytes = K * 3, 3 * 32 * 32 * 4
    for k, path in enumerate(paths, start=1):
        w = torch.load(path, weights_only=False)
        count = total // (4 * k)
        assert w.observed_tasks == list(range(k)) and w.cum_nc_per_task == [4, 8, 12] and w.n_total_memories == total
        assert w.exemplar_count == count and w.class_len == [count] * (4 * k)                  # K/m; every class has >= 12 images
        for c in range(4 * k):
            assert float(w.store_x[c * count:(c + 1) * count].abs().sum(dim=(1, 2, 3)).min()) > 0
        assert float(w.store_x[4 * k * count:].abs().sum()) == 0
        sizes = _storage_sizes(path)
        assert 4 * k * count * row_bytes in sizes and 4 * k * count * 12 * 4 in sizes             # stored rows and their targets
        if 4 * k * count < total:
            assert total * row_bytes not in sizes
        if k > 1:
            assert w.last_path == "fused"
        x = torch.randn(5, 3, 32, 32, device="cuda")
        code = w(x, k - 1)
        assert code.shape == (5, 12) and bool((code.sum(1) == 1).all()) and bool((code[:, 4 * (k - 1):4 * k].sum(1) == 1).all())
        if k < 3:
            nxt = w(x, k)                                                                        # no exemplars of that task yet
            assert bool((nxt[:, 4 * k:4 * (k + 1)] == 0.25).all()) and bool((nxt[:, :4 * k] < -1e10).all())
