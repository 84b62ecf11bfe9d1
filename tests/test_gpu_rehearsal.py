"""Rehearsal baselines on the MI355X: the segmented cross-entropy against a float64 torch restatement, the batch assembly
against torch.cat / index_select, the fused step against the segmented one at the task-10 shape of small_VGG9_cl_128_128,
and a replay of fixture G35 (tests/golden/make_g35.py) runs a / b / c with the recorded dropout masks."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g35_common as I  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _segs_dev(segs):
    """clhip_loss_segment rows of kind 0 (cross-entropy)."""
    host = np.zeros((len(segs), 6), dtype=np.int32)
    for i, (r0, r1, o, nc, sc) in enumerate(segs):
        host[i, :4] = (r0, r1, o, nc)
        host[i, 4] = np.array([sc], dtype=np.float32).view(np.int32)[0]
    return torch.from_numpy(host.reshape(-1)).to(DEV)


def _ce_ref(z, y, segs):
    z = z.double().cpu()
    y = y.cpu()
    loss = torch.zeros((), dtype=torch.float64)
    dz = torch.zeros_like(z)
    hits = 0
    for g, (r0, r1, o, nc, sc) in enumerate(segs):
        zs = z[r0:r1, o:o + nc]
        lp = torch.log_softmax(zs, 1)
        ce = -lp.gather(1, y[r0:r1, None])[:, 0]
        loss += sc * ce.mean()
        d = lp.exp()
        d[torch.arange(r1 - r0), y[r0:r1]] -= 1
        dz[r0:r1, o:o + nc] = d * (sc / (r1 - r0))
        if g == 0:
            hits = int((zs.argmax(1) == y[r0:r1]).sum())
    return loss, dz, hits


@pytest.mark.parametrize("N", [7, 268, 1024])
def test_segmented_ce_matches_f64(N):
    from clsurvey_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(N)
    ld = 200
    B = max(1, (N * 3) // 4)
    cuts = [B] + sorted(set(int(v) for v in torch.randint(B + 1, N, (5,), generator=gen).tolist())) + [N] if N > B + 1 else [B, N]
    slices = [(0, 20), (20, 100), (120, 70), (190, 10), (40, 65), (100, 20)]
    segs = [(0, B, 20, 100, 1.0)]
    bounds = [B] + [c for c in cuts[1:] if c > B]
    for i in range(len(bounds) - 1):
        o, nc = slices[i % len(slices)]
        segs.append((bounds[i], bounds[i + 1], o, nc, 1.0 / (len(bounds) - 1)))
    z = (torch.randn(N, ld, generator=gen) * 3).to(DEV)
    y = torch.empty(N, dtype=torch.int64)
    for r0, r1, o, nc, _ in segs:
        y[r0:r1] = torch.randint(0, nc, (r1 - r0,), generator=gen)
    y = y.to(DEV)
    sd = _segs_dev(segs)
    outs = []
    for _ in range(2):
        dz = torch.full((N, ld), 7.0, device=DEV)
        loss = torch.zeros(1, device=DEV)
        stats = torch.zeros(2, dtype=torch.float64, device=DEV)
        assert L.clhip_loss_segments(z.data_ptr(), y.data_ptr(), None, 0, N, ld, sd.data_ptr(), len(segs), 1.0, dz.data_ptr(),
                                     loss.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        outs.append((loss.cpu(), dz.cpu(), stats.cpu()))
    lref, dref, href = _ce_ref(z, y, segs)
    loss, dz, stats = outs[0]
    assert abs(float(loss) - float(lref)) <= 1e-6 * abs(float(lref))
    mask = dref != 0
    assert (dz[~mask] == 0).all()
    assert float((dz.double() - dref).abs().max()) <= 1e-6
    assert int(stats[1]) == href
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_mixed_table_segments_depend_on_their_own_rows_only():
    """N = 70, ld = 200: segment 0 of kind 0 (40 rows, 20 classes), a kind-0 chunk of 13 rows over 65 classes and a kind-1
    chunk of 17 rows over 20 classes (both sides of the 64-class boundary in one table).  Loss, gradient rows and hits of the
    kind-0 segments are bitwise those of a call that holds only them (same row numbers), the kind-1 rows bitwise those of a
    call that holds only that segment.  The kind-1 targets are the logits plus a fixed perturbation, so its KL is positive
    (checked in float64 on the host) and the gate stays open."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(70)
    N, ld, T = 70, 200, 2.0
    z = torch.randn(N, ld, generator=gen) * 3
    tg = z + 0.5 * torch.randn(N, ld, generator=gen)
    ce, kd = [(0, 40, 180, 20, 1.0, 0), (40, 53, 100, 65, 0.5, 0)], (53, 70, 20, 20, 2.75, 1)
    y = torch.zeros(N, dtype=torch.int64)
    for r0, r1, _, nc, _, _ in ce:
        y[r0:r1] = torch.randint(0, nc, (r1 - r0,), generator=gen)
    kl = torch.nn.KLDivLoss(reduction="batchmean")(torch.log_softmax(z[53:70, 20:40].double() / T, 1),
                                                   torch.softmax(tg[53:70, 20:40].double() / T, 1)) * T ** 2
    assert float(kl) > 1e-3
    z, tg, y = z.to(DEV), tg.to(DEV), y.to(DEV)

    def run(segs):
        stats = torch.zeros(2, dtype=torch.float64, device=DEV)
        loss, dz = ops.loss_segments(z, y, tg, ops.loss_segment_table(segs, DEV), len(segs), T, stats)
        return loss.cpu(), dz.cpu(), stats.cpu()
    loss_all, dz_all, st_all = run(ce + [kd])
    loss_ce, dz_ce, st_ce = run(ce)
    loss_kd, dz_kd, _ = run([kd])
    assert torch.equal(dz_all[:53], dz_ce[:53]) and float(dz_ce[:53].abs().max()) > 0
    assert torch.equal(dz_all[53:], dz_kd[53:]) and float(dz_kd[53:].abs().max()) > 0
    assert float(dz_ce[53:].abs().max()) == 0 and float(dz_kd[:53].abs().max()) == 0
    assert torch.equal(st_all[1], st_ce[1]) and int(st_ce[1]) == int((z[:40, 180:].argmax(1) == y[:40]).sum())
    assert float(loss_kd) > 0
    # the loss is one f32 rounding of the in-order f64 sum of the segments' values.  With the kind-1 segment at scale 0 its
    # value is +0.0 and the sum is that of the kind-0 call: bitwise.  At its own scale the three roundings (this loss, the
    # kind-0 call's, the kind-1 call's; all values positive) are half an ulp of the largest each: 1.5 * 2^-23 relative.
    assert torch.equal(run(ce + [kd[:4] + (0.0, 1)])[0], loss_ce)
    assert abs(float(loss_all) - (float(loss_ce) + float(loss_kd))) <= 1.5 * 2 ** -23 * float(loss_all)


def test_assemble_is_bitwise():
    from clsurvey_amd import _lib
    L = _lib.lib()
    row = (3, 64, 64)
    rows = 40
    store = torch.randn((rows,) + row, device=DEV)
    store_y = torch.randint(0, 20, (rows,), device=DEV)
    x = torch.randn((9,) + row, device=DEV)
    y = torch.randint(0, 20, (9,), device=DEV)
    gather = torch.tensor([3, 17, 0, 39, 17, 8], dtype=torch.int32, device=DEV)
    exp_store, exp_sy = store.clone(), store_y.clone()
    exp_store[20:25], exp_sy[20:25] = x[:5], y[:5]
    xm = torch.empty((15,) + row, device=DEV)
    ym = torch.empty(15, dtype=torch.int64, device=DEV)
    n = int(np.prod(row))
    assert L.clhip_rehearsal_assemble(x.data_ptr(), y.data_ptr(), 9, n, store.data_ptr(), store_y.data_ptr(), rows, 20, 5,
                                      gather.data_ptr(), 6, xm.data_ptr(), ym.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    gl = gather.long()
    assert torch.equal(store, exp_store) and torch.equal(store_y, exp_sy)
    assert torch.equal(xm, torch.cat([x, exp_store.index_select(0, gl)]))
    assert torch.equal(ym, torch.cat([y, exp_sy.index_select(0, gl)]))


def test_assemble_scalar_path_is_bitwise():
    """Rows of 3x7x5 floats (not a multiple of 4) and offset views: the kernel's element-wise copy path."""
    from clsurvey_amd import _lib
    L = _lib.lib()
    row = (3, 7, 5)
    n = int(np.prod(row))
    store_flat = torch.randn(12 * n + 1, device=DEV)
    store = store_flat[1:].view((12,) + row)                    # 4-byte offset: not 16-byte aligned
    store_y = torch.randint(0, 20, (12,), device=DEV)
    x = torch.randn((4,) + row, device=DEV)
    y = torch.randint(0, 20, (4,), device=DEV)
    gather = torch.tensor([11, 0, 5], dtype=torch.int32, device=DEV)
    exp_store, exp_sy = store.clone(), store_y.clone()
    exp_store[6:9], exp_sy[6:9] = x[:3], y[:3]
    before = store_flat[0].clone()
    xm = torch.empty((7,) + row, device=DEV)
    ym = torch.empty(7, dtype=torch.int64, device=DEV)
    assert L.clhip_rehearsal_assemble(x.data_ptr(), y.data_ptr(), 4, n, store.data_ptr(), store_y.data_ptr(), 12, 6, 3,
                                      gather.data_ptr(), 3, xm.data_ptr(), ym.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    gl = gather.long()
    assert torch.equal(store, exp_store) and torch.equal(store_y, exp_sy) and torch.equal(store_flat[0], before)
    assert torch.equal(xm, torch.cat([x, exp_store.index_select(0, gl)]))
    assert torch.equal(ym, torch.cat([y, exp_sy.index_select(0, gl)]))


def test_full_mode_compaction_is_bitwise():
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.full_mem_mode, w.n_tasks, w.n_total_memories, w.n_memories = True, 4, 40, 20
    w.observed_tasks, w.old_task, w.mem_cnt, w.filled = [0, 1], 1, 0, [20, 17, 0, 0]
    w.store_x = torch.randn(40, 3, 8, 8, device=DEV)
    w.store_y = torch.randint(0, 9, (40,), device=DEV)
    before_x, before_y = w.store_x.clone(), w.store_y.clone()
    w.switch_task(2)                        # 40 // 3 = 13 per task
    assert w.n_memories == 13 and w.filled[:2] == [13, 13]
    assert torch.equal(w.store_x[:13], before_x[:13]) and torch.equal(w.store_x[13:26], before_x[20:33])
    assert torch.equal(w.store_y[13:26], before_y[20:33])


def _task10_wrapper(force_segmented):
    from clsurvey_amd import models
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    torch.manual_seed(5)
    net = replace_head(models.parse_model_name("small_VGG9_cl_128_128", (64, 64), 20), 200)
    w = RehearsalNet(net, 200, 10, [20] * 10, 450, 0.0, 0.0, False, 268, (3, 64, 64), "cuda")
    w.init_setup(lr=0.0, weight_decay=0.0, n_append=68, chunk_size=132)
    gen = torch.Generator().manual_seed(9)
    w.store_x[:9 * 450] = torch.randn((9 * 450, 3, 64, 64), generator=gen).to(DEV)
    w.store_y[:9 * 450] = torch.randint(0, 20, (9 * 450,), generator=gen).to(DEV)
    w.observed_tasks, w.old_task, w.filled = list(range(9)), 8, [450] * 9 + [0]
    w.force_segmented = force_segmented
    masks = {li: (torch.rand(w.engine.in_elems[li], generator=gen) < 0.5).float().mul(2).to(DEV) for li in w.engine.drops}
    w._draw_mask = lambda li, n, p: masks[li]
    return w


def test_fused_step_matches_segmented_step_task10():
    """200 current images + 68 exemplars of 9 tasks (N = 268, shared mask rows): one fused pass against one pass per
    segment accumulated with clhip_axpy."""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((200, 3, 64, 64), generator=gen).to(DEV)
    y = torch.randint(0, 20, (200,), generator=gen).to(DEV)
    res = []
    for seg in (False, True):
        w = _task10_wrapper(seg)
        random.seed(3)
        torch.manual_seed(4)
        loss, hits = w.observe_FT(x, 9, y)
        torch.cuda.synchronize()
        assert w.last_path == ("segmented" if seg else "fused")
        res.append((float(loss), int(hits), w.A.grad.clone()))
    (lf, hf, gf), (ls, hs, gs) = res
    assert abs(lf - ls) <= 1e-5 * abs(ls)
    assert hf == hs
    assert rel_err(gf, gs) <= 1e-3


@pytest.mark.parametrize("tag", sorted(I.RUNS))
def test_g35_replay(tag):
    """Runs a / b / c of G35 with the recorded masks: losses within 3e-4, hits and memory labels exact, parameters at the
    end of each task rel_err <= 1e-3; run c (BatchNorm) takes the segmented path."""
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    spec = I.RUNS[tag]
    with open(os.path.join(HERE, "golden", "G35_rehearsal_baselines.json")) as f:
        steps = json.load(f)["runs"][tag]
    npz = np.load(os.path.join(HERE, "golden", "G35_rehearsal_baselines.npz"))
    net = replace_head(I.make_net(spec["bn"]), I.N_OUT)
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.from_numpy(npz["%s_p0_%d" % (tag, i)]))
    rows = I.B + max(a for a, _ in spec["append"])
    w = RehearsalNet(net, I.N_OUT, I.N_TASKS, I.NC_PER_TASK, spec["n_memories"], I.LR, I.WD, spec["full"], rows,
                     (3, I.HW, I.HW), "cuda")
    data = I.batches(spec["seed"] + 4)
    torch.manual_seed(spec["seed"] + 2)
    random.seed(spec["seed"] + 3)
    k = 0
    for t in range(I.N_TASKS):
        n_append, chunk = spec["append"][t]
        w.init_setup(lr=I.LR, weight_decay=I.WD, n_append=n_append, chunk_size=chunk)
        for _ in range(I.STEPS):
            rec = steps[k]
            ref_masks = [torch.from_numpy(npz[key]).to(DEV) for key in sorted(
                (kk for kk in npz.files if kk.startswith("%s_s%d_mask" % (tag, k))), key=lambda s: int(s.rsplit("mask", 1)[1]))]
            lis = sorted(w.engine.drops)
            w._draw_mask = lambda li, n, p, _m=dict(zip(lis, ref_masks)): _m[li]
            x, y = (torch.from_numpy(a).to(DEV) for a in data[k])
            loss, hits = w.observe_FT(x, t, y)
            assert abs(float(loss) - rec["loss"]) <= 3e-4 * abs(rec["loss"]), (tag, k, float(loss), rec["loss"])
            assert int(hits) == rec["hits"], (tag, k)
            assert (w.mem_cnt, w.n_memories) == (rec["mem_cnt"], rec["n_memories"])
            ref_labels = npz["%s_s%d_mem_labels" % (tag, k)]
            for task in w.observed_tasks:
                f, base = w.filled[task], task * w.n_memories
                assert (w.store_y[base:base + f].cpu().numpy() == ref_labels[task, :f]).all(), (tag, k, task)
            assert w.last_path == ("segmented" if spec["bn"] else "fused")
            k += 1
        for i, p in enumerate(net.parameters()):
            # (a conv bias in front of a BatchNorm has zero gradient in exact arithmetic: it moves by round-off alone, ~1e-11
            # here, so its error is taken against a 1e-6 floor instead of its own magnitude)
            ref = torch.from_numpy(npz["%s_p_task%d_%d" % (tag, t, i)])
            err = float((p.data.double().cpu() - ref.double()).abs().max())
            assert err <= 1e-3 * max(float(ref.abs().max()), 1e-6), (tag, t, i, err)
    # pickling carries the observed rows only and reloads
    import io
    buf = io.BytesIO()
    torch.save(w, buf)
    buf.seek(0)
    w2 = torch.load(buf, weights_only=False)
    assert w2.store_x.shape == w.store_x.shape and torch.equal(w2.store_y, w.store_y)
    assert w.__getstate__()["_rows_x"].shape[0] == (max(w.observed_tasks) + 1) * w.n_memories


def _storage_sizes(path):
    """Byte sizes of the tensor storages inside a torch.save archive."""
    import zipfile
    with zipfile.ZipFile(path) as z:
        return sorted(i.file_size for i in z.infolist() if "/data/" in i.filename and not i.filename.endswith(".pkl"))


@pytest.mark.parametrize("name", ["finetuning_rehearsal_partial_mem", "finetuning_rehearsal_full_mem"])
def test_rehearsal_baseline_through_driver(tmp_path, name):
    """Both methods through the driver on three tiny tasks with --test --mem_per_task K (grid over two LRs per task; every
    memory fills in the first epoch): results layout, the saved wrappers reload and evaluate, full-mode n_memories =
    total // tasks seen, and the pickles carry the rows of the observed tasks only."""
    import glob
    from clsurvey_amd.framework import driver
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import method as M
    from clsurvey_amd import models
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
    K = 24
    argv = ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "6", "--batch_size", "40", "--saving_freq",
            "100", "--method_name", name, "--results_root", root, "--test", "--mem_per_task", str(K)]
    out = driver.main(argv, method=M.parse(name), dataset=ds)
    res = out["results"]
    assert sorted(res) == [0, 1, 2]
    for i in res:
        assert len(res[i]["seq_res"][i]) == 3 - i
        assert all(0.0 <= a <= 100.0 for a in res[i]["seq_res"][i])
    assert res[0]["seq_res"][0][0] > 30.0, res
    full = name.endswith("full_mem")
    total = K * 3
    row_bytes = 3 * 32 * 32 * 4
    paths = out["model_paths"]
    assert len(paths) == 3
    for k, path in enumerate(paths, start=1):
        w = torch.load(path, weights_only=False)
        assert w.observed_tasks == list(range(k)) and w.cum_nc_per_task == [4, 8, 12]
        assert w.full_mem_mode == full and w.last_path == "fused"
        n = total // k if full else K
        assert w.n_memories == n
        assert all(f == n for f in w.filled[:k]) and all(f == 0 for f in w.filled[k:])     # every memory filled
        for task in range(k):
            assert float(w.store_x[task * n:(task + 1) * n].abs().sum()) > 0
        assert float(w.store_x[k * n:].abs().sum()) == 0
        sizes = _storage_sizes(path)
        assert k * n * row_bytes in sizes                     # the observed rows
        if k * n < total:
            assert total * row_bytes not in sizes              # never the whole store
        x = torch.randn(5, 3, 32, 32, device="cuda")
        lo = w(x, k - 1)
        o1, o2 = 4 * (k - 1), 4 * k
        assert lo.shape == (5, 12) and bool((lo[:, :o1] < -1e10).all()) and bool((lo[:, o2:] < -1e10).all())
        assert bool((lo[:, o1:o2] > -1e10).all())
    assert glob.glob(os.path.join(out["manager"].parent_exp_dir, "task_3", "TASK_TRAINING"))
