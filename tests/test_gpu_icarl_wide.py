"""Herding above 4096 features on the MI355X (clhip_icarl_herd_wide, F <= 16384): the wide entry against the narrow one wherever
both accept F (rankings bitwise equal, no gap condition: one pick-loop body serves both), against the torch restatement of
tests/test_gpu_icarl.py above 4096, its determinism and refusals, the nearest-mean kernel at the new widths, IcarlNet at F = 8192
in crop and in frame mode, and ICARL through the driver on wide_VGG9 at 64 x 64."""
import functools
import io
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _pattern(n, F, gen):
    """test_herding_matches_torch_at_realistic_size's features: a ReLU of a rank-3 pattern plus noise."""
    return torch.relu(torch.randn((n, 3), generator=gen) @ torch.randn((3, F), generator=gen) + 0.05 * torch.randn((n, F), generator=gen))


def _ranges(sizes):
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(bounds[c]), int(bounds[c + 1])) for c in range(len(sizes))]


def _weights(sizes, batch):
    from clsurvey_amd.methods.icarl import mean_weights
    return torch.from_numpy(np.concatenate([mean_weights(n, batch) for n in sizes]))


def _both(f, w, ranges, ks):
    """(narrow, wide) flat rankings of the same device tensors, on the CPU."""
    from clsurvey_amd import ops
    narrow, offs = ops.icarl_herd(f, w, ranges, ks, flat=True, wide=False)
    wide, offs_w = ops.icarl_herd(f, w, ranges, ks, flat=True, wide=True)
    assert list(offs) == list(offs_w)
    return narrow.cpu(), wide.cpu(), offs


# --------------------------------------------------------------------------- 1. wide == narrow where both exist
SIZES = [1, 5, 33, 137, 400, 9]          # one row; fewer rows than waves; crosses a `taken` word; odd; the realistic size; k = 0
PICKS = [1, 5, 33, 40, 60, 0]            # k = n three times (33 of 33 fills a taken word and a bit), k = 0 last: out_off 0, 1, 6, 39, 79, 139


@functools.lru_cache(maxsize=None)
def _six_classes(F):
    """Made once per width and never written to."""
    gen = torch.Generator().manual_seed(100 + F)
    return _pattern(sum(SIZES), F, gen), _weights(SIZES, 64)


@pytest.mark.parametrize("F", [1, 8, 260, 2048, 4096])
def test_wide_equals_narrow(F):
    """Six classes in one launch.  F = 1 takes the scalar path, the others the vector path: 8 leaves 62 lanes idle, 260 is 65
    float4 steps (one more than the lanes), 4096 is the narrow entry's limit.  No gap condition: the costs are the same
    expressions in the same order, so near-ties resolve alike."""
    f, w = _six_classes(F)
    narrow, wide, offs = _both(f.to(DEV), w.to(DEV), _ranges(SIZES), PICKS)
    assert torch.equal(narrow, wide)
    assert list(offs) == [0, 1, 6, 39, 79, 139, 139]
    for c, (n, k) in enumerate(zip(SIZES, PICKS)):
        r = wide[int(offs[c]):int(offs[c + 1])].tolist()
        assert len(r) == k and len(set(r)) == k and all(0 <= v < n for v in r), c      # relative to row_begin, no row twice
    assert sorted(wide[6:39].tolist()) == list(range(33))


@pytest.mark.parametrize("F", [8, 2048])
def test_wide_equals_narrow_on_the_scalar_path_of_unaligned_features(F):
    """F % 4 == 0 but feats 4 bytes off a 16-byte boundary: both entries take the scalar path."""
    sizes, ks = [33, 70], [20, 33]
    gen = torch.Generator().manual_seed(7 + F)
    n = sum(sizes)
    buf = torch.zeros(n * F + 4, device=DEV)
    f = buf[1:1 + n * F].view(n, F)
    f.copy_(_pattern(n, F, gen))
    assert f.data_ptr() % 16 == 4 and f.is_contiguous()
    w = _weights(sizes, 64).to(DEV)
    narrow, wide, _ = _both(f, w, _ranges(sizes), ks)
    assert torch.equal(narrow, wide)
    aligned_n, aligned_w, _ = _both(f.clone(), w, _ranges(sizes), ks)        # the vector path sums in another order: only
    assert torch.equal(aligned_n, aligned_w)                                 # wide against narrow is claimed, path by path


@pytest.mark.parametrize("F", [8, 260])
def test_duplicated_rows_tie_exactly_and_the_lower_row_comes_first(F):
    gen = torch.Generator().manual_seed(11 + F)
    sizes = [20, 70]
    f = _pattern(sum(sizes), F, gen)
    f[7] = f[3]                                       # class 0: rows 3 and 7
    f[20 + 69] = f[20 + 2]                            # class 1: rows 2 and 69 (different waves: 2 and 69 % 16 = 5)
    w = _weights(sizes, 64)
    narrow, wide, offs = _both(f.to(DEV), w.to(DEV), _ranges(sizes), sizes)             # k = n: every row is ranked
    assert torch.equal(narrow, wide)
    for r in (narrow, wide):
        r0, r1 = r[:20].tolist(), r[20:].tolist()
        assert r0.index(3) < r0.index(7) and r1.index(2) < r1.index(69)


def test_130_one_row_classes_make_two_launches():
    from clsurvey_amd import ops
    assert ops.ICARL_MAX_CLASSES == 128
    gen = torch.Generator().manual_seed(13)
    f = _pattern(130, 260, gen).to(DEV)
    w = torch.ones(130, device=DEV)
    narrow, wide, offs = _both(f, w, [(i, i + 1) for i in range(130)], [1] * 130)
    assert torch.equal(narrow, wide) and wide.tolist() == [0] * 130 and list(offs) == list(range(131))


# --------------------------------------------------------------------------- 2. against the torch restatement above 4096
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


@pytest.mark.parametrize("F,seed", [(4097, 38), (4100, 38), (8192, 42), (16384, 39)])
def test_wide_herding_matches_torch_above_4096(F, seed):
    """Classes of 130 and 47 rows, 30 and 12 picks, mean weights of batch 64; 4097 is the first width of the wide entry (scalar),
    4100 its first vector width, 8192 and 16384 the wide and the deep model's.  The gap condition (>= 1e-4 relative at every
    pick) is asserted on the restatement before the device is asked.  Gaps of the restatement on a CPU (class of 130, class of
    47): 4097 / 38: 4.7e-4, 2.2e-4; 4100 / 38: 1.3e-3, 2.4e-3; 8192 / 42: 1.6e-3, 1.3e-3 (seed 39 gives 1.04e-4 there, too
    close to the condition to rest a test on); 16384 / 39: 2.7e-4, 5.6e-4."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(seed)
    sizes, ks = [130, 47], [30, 12]
    f = _pattern(sum(sizes), F, gen)
    w = _weights(sizes, 64)
    want, lo = [], 0
    for n, k in zip(sizes, ks):
        rank, gap = _herd_restatement(f[lo:lo + n], w[lo:lo + n], k)
        print("F %d class of %d: restatement gap %.3g" % (F, n, gap))
        assert gap >= 1e-4, "restatement gap %.3g: change the seed of this test's data" % gap
        want.append(rank)
        lo += n
    got = ops.icarl_herd(f.to(DEV), w.to(DEV), _ranges(sizes), ks)           # wide=None: chosen by width
    assert [g.cpu().tolist() for g in got] == want


# --------------------------------------------------------------------------- 3. determinism, workspace, limit
def test_two_calls_give_the_same_ranking():
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(17)
    sizes, ks = [130, 47], [30, 12]
    f, w = _pattern(sum(sizes), 8192, gen).to(DEV), _weights(sizes, 64).to(DEV)
    a, _ = ops.icarl_herd(f, w, _ranges(sizes), ks, flat=True)
    ops.workspace(1, f.device, "icarl_herd").fill_(0xFF)                         # what an earlier call left in the workspace does not matter
    b, _ = ops.icarl_herd(f, w, _ranges(sizes), ks, flat=True)
    assert torch.equal(a, b) and a.shape[0] == 42


def test_short_workspace_and_16385_features_are_refused_before_any_launch():
    from clsurvey_amd import _lib, ops
    L = _lib.lib()
    F = 4100
    f, w = torch.ones((4, F), device=DEV), torch.full((4,), 0.25, device=DEV)
    tab = (_lib.IcarlClass * 1)()
    tab[0].row_begin, tab[0].row_end, tab[0].k, tab[0].out_off = 0, 4, 2, 0
    need = L.clhip_icarl_herd_wide_ws(1, F)
    assert need == 2 * F * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ranking = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_ptr, ws_bytes):
        return L.clhip_icarl_herd_wide(f.data_ptr(), 4, F, w.data_ptr(), tab, 1, ranking.data_ptr(), 2, ws_ptr, ws_bytes, stream)

    for args in ((ws.data_ptr(), need - 1), (None, need)):
        with pytest.raises(_lib.ClhipError, match="CLHIP_EINVAL"):
            _lib.check(call(*args), "clhip_icarl_herd_wide")
    torch.cuda.synchronize()
    assert ranking.tolist() == [-7, -7] and int(ws.sum()) == 0                # nothing ran
    _lib.check(call(ws.data_ptr(), need), "clhip_icarl_herd_wide")
    assert ranking.tolist() == [0, 1]                                         # four equal rows: the lowest untaken row every time
    wide = torch.ones((4, 16385), device=DEV)
    for flag in (None, True):
        with pytest.raises(_lib.ClhipError, match="clhip_icarl_herd_wide: CLHIP_EINVAL"):
            ops.icarl_herd(wide, w, [(0, 4)], [2], wide=flag)
    with pytest.raises(_lib.ClhipError, match="clhip_icarl_herd: CLHIP_EINVAL"):
        ops.icarl_herd(f, w, [(0, 4)], [2], wide=False)                       # the narrow entry keeps its limit


# --------------------------------------------------------------------------- 4. nearest mean at the new widths
@pytest.mark.parametrize("F", [4097, 8192, 16384])
def test_nme_matches_torch_with_ties_at_wide_features(F):
    """tests/test_gpu_icarl.py::test_nme_matches_torch_with_ties at the widths this change opens (it runs at F = 256).  The NME
    kernel has no width limit and is not changed here: this test passes without the wide herding entry too."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(5)
    N, C, o1, n_out = 37, 5, 4, 12
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


# --------------------------------------------------------------------------- 5, 6. the wrapper at F = 8192
HW, NCLS, N_TASKS, PER_CLASS, N_MEM, HERD_BATCH, ENGINE_BATCH, MARGIN = 64, 4, 3, 24, 16, 10, 32, 8
F_WRAP = 32 * 16 * 16


def _net():
    from clsurvey_amd.models import VGGSlim
    torch.manual_seed(5)
    return VGGSlim(cfg=[16, "M", 32, "M"], num_classes=NCLS, classifier_inputdim=F_WRAP, classifier_dim1=32, classifier_dim2=32)


def _wrapper(spec=None, frame_shape=None):
    from clsurvey_amd.methods.icarl import IcarlNet
    kw = dict(exemplar_transform=spec, frame_shape=frame_shape) if spec is not None else {}
    return IcarlNet(_net(), N_TASKS * NCLS, N_TASKS, [NCLS] * N_TASKS, N_MEM, lr=0.02, weight_decay=1e-4, memory_strength=1.0,
                    batch_size=ENGINE_BATCH, in_shape=(3, HW, HW), device="cuda", **kw)


@functools.lru_cache(maxsize=None)
def _task_tensors(t, hw):
    """About 24 images a class (22, 23, 25, 26), labels shuffled; on the device, never written to."""
    gen = torch.Generator().manual_seed(300 + t)
    y = torch.cat([torch.full((n,), c, dtype=torch.int64) for c, n in enumerate((22, 23, 25, 26))])
    y = y[torch.randperm(y.shape[0], generator=gen)]
    x = torch.randn((y.shape[0], 3, hw, hw), generator=gen) + (y[:, None, None, None] - 1.5) * 0.5
    return x.to(DEV), y.to(DEV)


def _herd_args(dset):
    return types.SimpleNamespace(task_imgfolders={"train": dset}, batch_size=HERD_BATCH)


def _direct_ranking(w, crops, y):
    """ops.icarl_herd on w.features(crops) in class order, as manage_memory states it.  Returns (ranking, offs, order, bounds, ks)."""
    from clsurvey_amd import ops
    w.net.train(False)
    w._dropout(1)
    feats = w.features(crops)
    assert feats.shape[1] == F_WRAP == 8192
    order = torch.sort(y, stable=True)[1]
    sizes = torch.bincount(y, minlength=NCLS).cpu().tolist()
    ks = [min(w.exemplar_count, m) for m in sizes]
    ranking, offs = ops.icarl_herd(feats.index_select(0, order), _weights(sizes, HERD_BATCH).to(DEV), _ranges(sizes), ks, flat=True)
    return ranking, offs, order, np.concatenate([[0], np.cumsum(sizes)]), ks


def _winners(ranking, offs, order, bounds, c):
    return order[int(bounds[c]) + ranking[int(offs[c]):int(offs[c + 1])].long()]


def _probe_codes(w):
    probe = torch.randn((7, 3, HW, HW), generator=torch.Generator().manual_seed(77)).to(DEV)
    args = types.SimpleNamespace(batch_size=5)
    return [w(probe, t, args=args).cpu() for t in range(2)]


def _check_codes(codes):
    for t, code in enumerate(codes):
        assert code.shape == (7, N_TASKS * NCLS) and bool((code.sum(1) == 1).all())
        assert bool((code[:, NCLS * t:NCLS * (t + 1)].sum(1) == 1).all())        # 1-of-C inside the task's slice


def _roundtrip(w):
    buf = io.BytesIO()
    torch.save(w, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def test_wrapper_in_crop_mode_herds_8192_features():
    from clsurvey_amd.data import TensorTaskDataset
    from clsurvey_amd.methods.icarl import compute_offsets
    w = _wrapper()
    total = N_MEM * N_TASKS
    first = {}
    for t in range(2):
        x, y = _task_tensors(t, HW)
        w.manage_memory(t, _herd_args(TensorTaskDataset(x, y, [str(c) for c in range(NCLS)])))      # (does not raise)
        count = total // (NCLS * (t + 1))
        assert w.exemplar_count == count and w.class_len == [count] * (NCLS * (t + 1))              # K/m: 12, then 6
        ranking, offs, order, bounds, ks = _direct_ranking(w, x, y)
        assert torch.equal(ranking, w.last_ranking[0]) and list(offs) == list(w.last_ranking[1]) and ks == [count] * NCLS
        o1, _ = compute_offsets(t, w.cum_nc_per_task)
        wins = [_winners(ranking, offs, order, bounds, c) for c in range(NCLS)]
        for c in range(NCLS):
            r0, m = w._block(o1 + c)
            assert m == count and torch.equal(w.store_x[r0:r0 + m], x[wins[c]])                    # bitwise the ranked images
        if t == 0:
            first = {c: x[wins[c]][:total // (2 * NCLS)].clone() for c in range(NCLS)}
        targets = torch.cat([w.store_t[w._block(o1 + c)[0]:w._block(o1 + c)[0] + count] for c in range(NCLS)])
        assert torch.equal(targets, w.forward_training(x[torch.cat(wins)], t)) and float(targets[:, o1:o1 + NCLS].abs().sum()) > 0
    for c in range(NCLS):                                 # the second call kept the first 6 of every class of task 0
        r0, m = w._block(c)
        assert m == 6 and torch.equal(w.store_x[r0:r0 + m], first[c])
    assert float(w.store_x[2 * NCLS * 6:].abs().sum()) == 0
    codes = _probe_codes(w)
    _check_codes(codes)
    w2 = _roundtrip(w)
    assert w2.class_len == [6] * 8 and w2.exemplar_count == 6 and torch.equal(w2.store_x, w.store_x) and torch.equal(w2.store_t, w.store_t)
    for a, b in zip(codes, _probe_codes(w2)):
        assert torch.equal(a, b)


def test_wrapper_in_frame_mode_herds_8192_features():
    """RandomCropFlip on 72 x 72 frames with exemplar_transform set (--icarl_frames's path): the frames and extents are stored,
    last_ranking is the direct call on the features of the herding view (restated on the CPU by slicing)."""
    from clsurvey_amd.data import RandomCropFlip, TensorTaskDataset
    from clsurvey_amd.methods.icarl import VIEW_HERD, compute_offsets
    spec = RandomCropFlip((HW, HW), 0.5)
    side = HW + MARGIN
    w = _wrapper(spec, (3, side, side))
    assert tuple(w.store_x.shape) == (N_MEM * N_TASKS, 3, side, side)
    for t in range(2):
        x, y = _task_tensors(t, side)
        dset = TensorTaskDataset(x, y, [str(c) for c in range(NCLS)], transform=RandomCropFlip((HW, HW), 0.5))
        w.manage_memory(t, _herd_args(dset))
        n, count = len(dset), N_MEM * N_TASKS // (NCLS * (t + 1))
        assert w.exemplar_count == count and w.class_len == [count] * (NCLS * (t + 1))
        params = w.last_herd_params
        assert torch.equal(params, w.view_params(t, VIEW_HERD, w._full_ext(n))) and tuple(params.shape) == (n, 3)
        assert 0 < int(params[:, :2].max()) <= MARGIN and 0 < int(params[:, 2].sum()) < n
        xc = x.cpu()
        crops = torch.stack([xc[i, :, top:top + HW, left:left + HW].flip(-1) if flip else xc[i, :, top:top + HW, left:left + HW]
                             for i, (top, left, flip) in enumerate(params.tolist())]).to(DEV)
        ranking, offs, order, bounds, ks = _direct_ranking(w, crops, y)
        assert torch.equal(ranking, w.last_ranking[0]) and list(offs) == list(w.last_ranking[1])
        o1, _ = compute_offsets(t, w.cum_nc_per_task)
        for c in range(NCLS):
            r0, m = w._block(o1 + c)
            win = _winners(ranking, offs, order, bounds, c)
            assert m == count and torch.equal(w.store_x[r0:r0 + m], x[win])
            assert w.store_ext[r0:r0 + m].tolist() == [[side, side]] * m
    assert float(w.store_t[:2 * NCLS * 6].abs().sum()) > 0
    _check_codes(_probe_codes(w))


# --------------------------------------------------------------------------- 7. the driver
MODEL = "wide_VGG9_cl_128_128"


K_DRIVER = 8


def _drive(root, data_seed=7, init_seed=0):
    """An SI first-task dump, then 3 tasks of ICARL with --test on wide_VGG9 at 64 x 64; returns driver.main's result."""
    from clsurvey_amd import models
    from clsurvey_amd.framework import driver
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import method as M
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=3, classes_per_task=4, sizes=(64, 16, 16), hw=64, noise=0.4,
                               seed=data_seed, name="tiny3wide")
    torch.manual_seed(init_seed)
    base = models.parse_model_name(MODEL, (64, 64), 4)
    assert base.classifier[0].in_features == 8192
    for mod in base.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(base, os.path.join(root, "models", MODEL + ".pth.tar"))
    common = [MODEL, "--lr_grid", "1e-2", "--num_epochs", "2", "--batch_size", "16", "--saving_freq", "100"]
    driver.main(common + ["--method_name", "SI", "--results_root", root, "--runmode", "first_task_basemodel_dump"],
                method=M.parse("SI"), dataset=ds)
    icarl = M.parse("ICARL")
    icarl.static_hyperparams = {"mem_per_task": K_DRIVER}
    return driver.main(common + ["--method_name", "ICARL", "--results_root", root, "--test"], method=icarl, dataset=ds)


def test_icarl_through_the_driver_on_wide_vgg9(tmp_path):
    """tests/test_gpu_icarl.py::test_icarl_through_driver's route on wide_VGG9 at 64 x 64 (8192 features).  The image counts and
    epochs are shrunk, not the width: 64 / 16 / 16 images a task, 2 epochs, one learning rate, 8 exemplars a task (K/m = 6, 3, 2:
    below the smallest class of 64 labels drawn uniformly).  The three wrappers reload, exemplar_count and class_len follow K/m,
    the stored rows are not zero, the accuracies (nearest mean of exemplars) are finite and, as in the existing test, above 35 %
    on the task just learned (chance is 25 %).  Observed on an MI355X with (data seed, init seed) = (7, 0), (8, 1), (9, 2): 100 %
    on every task after every task, three times.  The prototypes of this sequence are far apart in the 8192 features even of
    a barely trained net (the training accuracy of these two epochs is 15 - 30 %), so the nearest mean does not depend on how
    far the training got."""
    out = _drive(str(tmp_path))
    res = out["results"]
    assert sorted(res) == [0, 1, 2]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("accuracies", {i: res[i]["seq_res"][i] for i in res})
    assert len(accs) > 0 and all(np.isfinite(a) and 0.0 <= a <= 100.0 for a in accs)
    assert all(res[i]["seq_res"][i][0] > 35.0 for i in res), res              # chance is 25 %
    paths = out["model_paths"]
    assert len(paths) == 3
    total = K_DRIVER * 3
    for k, path in enumerate(paths, start=1):
        w = torch.load(path, weights_only=False)
        count = total // (4 * k)
        assert w.engine.layer_input(w.fc_first, 1).shape[1] == 8192
        assert w.observed_tasks == list(range(k)) and w.n_total_memories == total
        assert w.exemplar_count == count and w.class_len == [count] * (4 * k)                  # K/m
        for c in range(4 * k):
            assert float(w.store_x[c * count:(c + 1) * count].abs().sum(dim=(1, 2, 3)).min()) > 0
        assert float(w.store_x[4 * k * count:].abs().sum()) == 0
