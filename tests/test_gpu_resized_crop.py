"""RandomResizedCrop + flip augmentation on the GPU: clhip_gather_tasks_resized_crop_flip against the fp64 restatement of its
formula (tests/resized_crop_ref.py) with ATen's own fp32 error as the yardstick, identity windows against the copying gather
(bitwise), determinism, the safety rule, the loaders against their host-recomputed tables, a spec without freedom as the
identity of a training epoch, and `--rnd_resized` through the driver."""
import functools
import os
import sys
from itertools import accumulate

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resized_crop_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 4.0          # the kernel's largest error may be this many times ATen's fp32 CPU error on the same cases (same precision;
#                       the rounding of the weights and the summation order differ)


def _tasks(T, C, Hs, Ws, seed):
    gen = torch.Generator().manual_seed(seed)
    sizes, ncls = ([5, 1, 7], [3, 2, 4]) if T == 3 else ([13], [9])
    xs = [torch.randn((n, C, Hs, Ws), generator=gen) for n in sizes]
    ys = [torch.randint(0, k, (n,), generator=gen) for n, k in zip(sizes, ncls)]
    shifts = [0] + list(accumulate(ncls))[:-1]
    return xs, ys, list(accumulate(sizes)), shifts


def _table(xs, ys, cum, shifts):
    from clsurvey_amd import ops
    dev_x, dev_y = [x.to(DEV) for x in xs], [y.to(DEV) for y in ys]
    return ops.task_table(dev_x, dev_y, cum, shifts, DEV), (dev_x, dev_y)          # (the table holds pointers: keep the tensors)


def _hand_made(Hs, Ws):
    """1 x 1 windows in two corners, the whole frame under both flips, and a window touching each border."""
    h, w = max(1, (2 * Hs) // 3), max(1, (2 * Ws) // 3)
    return [[0, 0, 1, 1, 0], [Hs - 1, Ws - 1, 1, 1, 1], [0, 0, Hs, Ws, 0], [0, 0, Hs, Ws, 1],
            [0, (Ws - w) // 2, h, w, 1], [Hs - h, (Ws - w) // 2, h, w, 0], [(Hs - h) // 2, 0, h, w, 1], [(Hs - h) // 2, Ws - w, h, w, 0]]


@functools.lru_cache(maxsize=None)
def _cases(C, Hs, Ws, th, tw):
    """The launches of one geometry, each with its fp64 restatement and ATen's fp32 result, computed once:
    [(xs, ys, cum, shifts, idx, params, want64, aten32)] for (T, B) in {1, 3} x {1, 37}."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    out = []
    for T in (1, 3):
        xs, ys, cum, shifts = _tasks(T, C, Hs, Ws, 100 * T + Hs + tw)
        frames = torch.cat(xs)
        for B in (1, 37):
            g = torch.Generator().manual_seed(B + T)
            if B == 1:
                idx, params = torch.tensor([cum[-1] - 1]), torch.tensor([[0, 0, Hs, Ws, 1]], dtype=torch.int32)
            else:
                hand = torch.tensor(_hand_made(Hs, Ws), dtype=torch.int32)
                drawn = draw_resized_crop_flip(B - len(hand), RandomResizedCropFlip((th, tw)), (Hs, Ws), g)
                params = torch.cat([hand, drawn])
                idx = torch.cat([torch.arange(cum[-1]), torch.randint(0, cum[-1], (B - cum[-1],), generator=g)])   # every sample, every task
            out.append((xs, ys, cum, shifts, idx, params, ref.restate(frames, idx, params, th, tw), ref.aten(frames, idx, params, th, tw)))
    return out


GEOMETRIES = [(1, 5, 7, 8, 8), (3, 40, 33, 8, 8), (2, 9, 9, 4, 12), (3, 64, 64, 56, 56), (2, 64, 64, 8, 8), (3, 12, 10, 5, 7)]
IDS = ["%dx%dx%d_to_%dx%d" % g for g in GEOMETRIES]


@pytest.mark.parametrize("C,Hs,Ws,th,tw", GEOMETRIES, ids=IDS)
def test_kernel_is_the_restatement_within_atens_own_error(C, Hs, Ws, th, tw):
    """Enlarging / shrinking with 11 taps / shrinking in y and enlarging in x / the Tiny-ImageNet shape / 17 taps / a width
    that takes the plain stores.  T = 1 and 3 tasks (label shifts, every task boundary), B = 1 and 37, windows of the default
    spec plus hand-made ones, both flips.  e_ref = ATen's fp32 CPU error against the fp64 restatement over these launches; the
    kernel's error over the same launches is at most MARGIN e_ref.  Labels are exact."""
    from clsurvey_amd import ops
    e_ref = e_kernel = 0.0
    for xs, ys, cum, shifts, idx, params, want, aten in _cases(C, Hs, Ws, th, tw):
        table, keep = _table(xs, ys, cum, shifts)
        x, y = ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV))
        assert tuple(x.shape) == (idx.shape[0], C, th, tw) and x.dtype == torch.float32
        assert torch.equal(y.cpu(), torch.cat([v + s for v, s in zip(ys, shifts)])[idx])
        e_kernel = max(e_kernel, float((x.cpu().double() - want).abs().max()))
        e_ref = max(e_ref, float((aten.double() - want).abs().max()))
    print("resized crop %s: kernel error %.3g, ATen fp32 error %.3g, ratio %.2f" % ((C, Hs, Ws, th, tw), e_kernel, e_ref, e_kernel / e_ref))
    assert e_ref > 0.0
    assert e_kernel <= MARGIN * e_ref


@pytest.mark.parametrize("C,Hs,Ws,th,tw", [(3, 20, 20, 16, 16), (3, 13, 11, 8, 7), (2, 40, 72, 36, 64), (1, 16, 16, 16, 16)],
                         ids=["20x20_to_16x16", "13x11_to_8x7", "40x72_to_36x64", "no_freedom"])
def test_identity_windows_are_the_copying_gather_bitwise(C, Hs, Ws, th, tw):
    """h == th and w == tw: one tap of weight exactly 1 per axis, so the bytes are those of clhip_gather_tasks_crop_flip for
    (top, left, flip).  -0.0 and an infinity beside the window survive (taps of weight 0 take no part)."""
    from clsurvey_amd import ops
    xs, ys, cum, shifts = _tasks(3, C, Hs, Ws, 7 + Hs)
    xs[0][0, 0, 0, 0] = -0.0
    xs[0][0, 0, 1, 1] = float("inf")
    xs[2][6, C - 1, Hs - 1, Ws - 1] = float("-inf")
    table, keep = _table(xs, ys, cum, shifts)
    mt, ml = Hs - th, Ws - tw
    idx = torch.tensor([0, 4, 5, 6, 12, 4, 9, 0, 12])
    p3 = torch.tensor([[0, 0, 0], [mt, ml, 1], [0, ml, 1], [mt, 0, 0], [mt, ml, 0], [mt // 2, min(1, ml), 0],
                       [min(1, mt), ml // 2, 1], [0, 0, 1], [mt, ml, 1]], dtype=torch.int32)
    p5 = torch.stack([p3[:, 0], p3[:, 1], torch.full((9,), th, dtype=torch.int32), torch.full((9,), tw, dtype=torch.int32), p3[:, 2]], 1)
    want, want_y = ops.gather_tasks_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), p3.to(DEV))
    got, got_y = ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), p5.contiguous().to(DEV))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_y, want_y)
    assert bool(torch.isinf(got).any())


def test_two_launches_are_bitwise_equal():
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = GEOMETRIES[3]
    xs, ys, cum, shifts, idx, params, want, _ = _cases(C, Hs, Ws, th, tw)[3]
    table, keep = _table(xs, ys, cum, shifts)
    a, ya = ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV))
    b, yb = ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ya, yb)


def test_unaligned_output_takes_the_plain_path():
    """tw % 4 == 0 but x_out 4 bytes off a 16-byte boundary: no vector stores, the same bytes, nothing before the buffer."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = GEOMETRIES[1]
    xs, ys, cum, shifts, idx, params, want, _ = _cases(C, Hs, Ws, th, tw)[3]
    table, keep = _table(xs, ys, cum, shifts)
    B = idx.shape[0]
    buf = torch.full((1 + B * C * th * tw + 3,), -7.0, device=DEV)
    assert buf[1:].data_ptr() % 16 == 4
    ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV), x_out=buf[1:])
    vec, _ = ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV))
    assert torch.equal(buf[1:1 + vec.numel()].view(torch.int32), vec.view(-1).view(torch.int32))
    assert float(buf[0]) == -7.0 and bool((buf[1 + vec.numel():] == -7.0).all())


def test_bad_rows_copy_nothing_and_get_label_minus_one():
    """The kernel's defined behaviour for a table the host would never upload, between good rows: sample number == total and
    -1, top and left below 0, a window past the bottom and past the right edge, h = 0, w = 0, flip = 2, h and w over
    CLHIP_RESIZE_MAX_RATIO times the output (inside the frame).  Those rows keep the sentinel; the good ones are what a launch of
    the good rows alone gives, and that is the restatement."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = 2, 20, 26, 2, 3
    xs, ys, cum, shifts = _tasks(3, C, Hs, Ws, 5)
    table, keep = _table(xs, ys, cum, shifts)
    rows = [(3, [1, 2, 10, 9, 1], True), (13, [0, 0, 4, 4, 0], False), (6, [4, 4, 16, 20, 0], True), (-1, [0, 0, 4, 4, 0], False),
            (5, [-1, 0, 4, 4, 0], False), (2, [0, -1, 4, 4, 1], False), (12, [0, 3, 5, 7, 1], True), (7, [17, 0, 4, 4, 0], False),
            (1, [0, 23, 4, 4, 0], False), (4, [2, 2, 0, 4, 0], False), (4, [2, 2, 4, 0, 1], False), (0, [2, 2, 2, 2, 0], True),
            (8, [2, 2, 4, 4, 2], False), (9, [0, 0, 17, 4, 0], False), (10, [0, 0, 4, 25, 1], False), (11, [19, 25, 1, 1, 1], True),
            (3, [0, 0, 4, 4, -1], False)]
    idx = torch.tensor([r[0] for r in rows])
    params = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    good = [k for k, r in enumerate(rows) if r[2]]
    bad = [k for k, r in enumerate(rows) if not r[2]]
    x = torch.full((len(rows), C, th, tw), -7.0, device=DEV)
    labels = torch.full((len(rows),), 99, dtype=torch.int64, device=DEV)
    ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV), x_out=x, labels_out=labels)
    alone, alone_y = ops.gather_tasks_resized_crop_flip(table, (C, Hs, Ws, th, tw), idx[good].to(DEV), params[good].to(DEV))
    x, labels = x.cpu(), labels.cpu()
    assert bool((x[bad] == -7.0).all()) and labels[bad].tolist() == [-1] * len(bad)
    assert torch.equal(x[good], alone.cpu()) and torch.equal(labels[good], alone_y.cpu())
    assert torch.equal(labels[good], torch.cat([v + s for v, s in zip(ys, shifts)])[idx[good]])
    frames = torch.cat(xs)
    want = ref.restate(frames, idx[good], params[good], th, tw)
    e_ref = float((ref.aten(frames, idx[good], params[good], th, tw).double() - want).abs().max())
    e_kernel = float((x[good].double() - want).abs().max())
    print("good rows between bad ones: kernel error %.3g, ATen fp32 error %.3g" % (e_kernel, e_ref))
    assert e_ref > 0.0 and e_kernel <= MARGIN * e_ref


def test_geometry_errors_are_einval_before_any_launch():
    from clsurvey_amd import _lib, ops
    xs, ys, cum, shifts = _tasks(3, 2, 20, 20, 5)
    table, keep = _table(xs, ys, cum, shifts)
    idx = torch.tensor([0, 1], device=DEV)
    params = torch.tensor([[0, 0, 4, 4, 0]] * 2, dtype=torch.int32, device=DEV)
    x = torch.full((2, 2, 16, 16), -7.0, device=DEV)
    for geometry in ((2, 0, 20, 16, 16), (2, 20, 0, 16, 16), (2, 20, 20, 0, 16), (2, 20, 20, 16, 0), (0, 20, 20, 16, 16), (2, 20, 20, -1, 16)):
        with pytest.raises(_lib.ClhipError, match="CLHIP_EINVAL"):
            ops.gather_tasks_resized_crop_flip(table, geometry, idx, params, x_out=x)
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())
    with pytest.raises(AssertionError):                                             # the crop gather's table has another shape
        ops.gather_tasks_resized_crop_flip(table, (2, 20, 20, 16, 16), idx, params[:, :3].contiguous())
    with pytest.raises(AssertionError):
        ops.gather_tasks_resized_crop_flip(table, (2, 20, 20, 16, 16), idx, params.long())
    with pytest.raises(RuntimeError):
        ops.gather_tasks_resized_crop_flip(table, (2, 20, 20, 16, 16), idx, params.cpu())
    x0, y0 = ops.gather_tasks_resized_crop_flip(table, (2, 20, 20, 16, 16), idx[:0], params[:0])
    assert tuple(x0.shape) == (0, 2, 16, 16) and tuple(y0.shape) == (0,)


# ---------------------------------------------------------------------------------------------- loaders
def _sequence(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=3, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                               name="rrc3", rnd_resized=4, **kw)
    return ds, [ds.get_task_dataset_path(str(t), rnd_transform=True) for t in (1, 2, 3)]


def _host_epoch(n, shuffle, spec, frame_hw):
    """What a loader does with the global generator and its base seed, restated: (order, parameter table)."""
    from clsurvey_amd.data import draw_resized_crop_flip
    base = int(torch.empty((), dtype=torch.int64).random_().item())
    perm = None
    if shuffle:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = draw_resized_crop_flip(n, spec, frame_hw, torch.Generator().manual_seed(base), order=perm)
    return (torch.arange(n) if perm is None else perm), table


@pytest.mark.parametrize("multi,shuffle", [(False, True), (False, False), (True, True)],
                         ids=["DeviceLoader-shuffle", "DeviceLoader-in_order", "MultiTaskLoader"])
def test_loader_serves_the_restatement_of_its_own_draws(tmp_path, multi, shuffle):
    from clsurvey_amd.data import DeviceLoader, MultiTaskLoader, RandomResizedCropFlip, TaskList, load_task_datasets
    _, paths = _sequence(str(tmp_path))
    tasks = [load_task_datasets(p, DEV)["train"] for p in paths]
    assert all(isinstance(t.transform, RandomResizedCropFlip) and t.x.is_cuda and tuple(t.x.shape) == (24, 3, 20, 20) for t in tasks)
    if multi:
        loader = MultiTaskLoader(TaskList(tasks), 7, shuffle, DEV)
        frames = torch.cat([t.x for t in tasks]).cpu()
        labels = torch.cat([t.y + s for t, s in zip(tasks, (0, 4, 8))]).cpu()
    else:
        loader = DeviceLoader(tasks[0], 7, shuffle, DEV)
        frames, labels = tasks[0].x.cpu(), tasks[0].y.cpu()
    n = frames.shape[0]
    assert tuple(loader.x.shape) == (0, 3, 16, 16) and len(loader) == (n + 6) // 7
    torch.manual_seed(3)
    got, served = [], []
    for x, y in loader:
        got.append((x, y))
        served.append((loader.last_idx.cpu(), loader.last_idx_host.clone()))
    after = torch.get_rng_state()
    torch.manual_seed(3)
    order, table = _host_epoch(n, shuffle, tasks[0].transform, (20, 20))
    assert torch.equal(after, torch.get_rng_state())
    assert [b[0].shape[0] for b in got] == [7] * (n // 7) + ([n % 7] if n % 7 else [])
    assert torch.equal(torch.cat([s[0] for s in served]), order) and torch.equal(torch.cat([s[1] for s in served]), order)
    assert torch.equal(torch.cat([b[1] for b in got]).cpu(), labels[order])
    want = ref.restate(frames, order, table, 16, 16)
    e_ref = float((ref.aten(frames, order, table, 16, 16).double() - want).abs().max())
    e_kernel = float((torch.cat([b[0] for b in got]).cpu().double() - want).abs().max())
    print("loader epoch: kernel error %.3g, ATen fp32 error %.3g" % (e_kernel, e_ref))
    assert e_ref > 0.0 and e_kernel <= MARGIN * e_ref
    assert len(set(map(tuple, table.tolist()))) > 5                                 # the draws do differ between positions
    if not shuffle:                                                                 # the next epoch: the same samples, other windows
        second = list(loader)
        a, b = torch.cat([v[0] for v in got]), torch.cat([v[0] for v in second])
        assert torch.equal(torch.cat([v[1] for v in second]).cpu(), labels)
        assert sum(int(not torch.equal(a[i], b[i])) for i in range(n)) > n // 2


def test_spec_without_freedom_serves_the_plain_loaders_epoch_and_trains_the_same_model(tmp_path):
    """scale = ratio = (1, 1), p = 0 on square frames of the output size: every window is the whole frame, every tap has weight
    1 — the batches are bitwise the plain loader's and one epoch of fine_tune_SGD ends at bitwise equal parameters."""
    from clsurvey_amd import models
    from clsurvey_amd.data import DeviceLoader, RandomResizedCropFlip, TensorTaskDataset, load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import finetune
    root = str(tmp_path)
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=1, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="mem1")
    dsets = load_task_datasets(ds.get_task_dataset_path("1"), DEV)
    torch.manual_seed(0)
    base = os.path.join(root, "base.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), base)
    params, epochs = [], []
    for tag in ("resized", "plain"):
        spec = RandomResizedCropFlip((32, 32), scale=(1, 1), ratio=(1, 1), p=0.0) if tag == "resized" else None
        per = {s: TensorTaskDataset(dsets[s].x, dsets[s].y, dsets[s].classes, transform=spec) for s in ("train", "val")}
        torch.manual_seed(7)
        loaders = {s: DeviceLoader(per[s], 40, True, DEV) for s in per}
        assert (loaders["train"].transform is not None) == (tag == "resized") and tuple(loaders["train"].x.shape[1:]) == (3, 32, 32)
        epochs.append([(x.clone(), y.clone()) for x, y in loaders["train"]])
        torch.manual_seed(7)
        model, _ = finetune.fine_tune_SGD(loaders, {s: len(per[s]) for s in per}, {s: [per[s].classes] for s in per},
                                          model_path=base, exp_dir=os.path.join(root, tag), num_epochs=1, lr=1e-2, device=DEV,
                                          batch_size=40)
        params.append([p.detach().clone() for p in model.parameters()])
    assert len(epochs[0]) == len(epochs[1]) == 2
    for (xa, ya), (xb, yb) in zip(*epochs):
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ya, yb)
    start = list(torch.load(base, weights_only=False).parameters())
    assert any(not torch.equal(a.cpu(), s) for a, s in zip(params[0], start))        # the epoch did train
    for a, b in zip(*params):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- through the driver
def _friendly_base_model(root):
    """As tests/test_gpu_framework.py: a kaiming classifier init, so that a few epochs move the loss."""
    from clsurvey_amd import models
    torch.manual_seed(0)
    m = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(m, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))


def _common(root, extra):
    return ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "3", "--batch_size", "40", "--saving_freq", "100",
            "--results_root", root, "--synthetic", "2,4,160,40,40,32"] + extra


def _ewc(root, extra):
    from clsurvey_amd.framework import driver
    _friendly_base_model(root)
    driver.main(_common(root, extra) + ["--method_name", "SI", "--runmode", "first_task_basemodel_dump"])
    return driver.main(_common(root, extra) + ["--method_name", "EWC", "--test", "--drop_margin", "0.05"])


def _model_files(root):
    out = {}
    for d, _, files in os.walk(os.path.join(root, "train")):
        for f in files:
            if f == "best_model.pth.tar":
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def _finite(accs):
    return len(accs) > 0 and all(a == a and 0.0 <= a <= 100.0 for a in accs)


def test_ewc_through_the_driver_on_resampled_tasks(tmp_path):
    """SI dump, LR grid, a Fisher pass over a resampling reg_sets loader, evaluation on the static test split."""
    from clsurvey_amd.data import RandomResizedCropFlip
    root = str(tmp_path)
    out = _ewc(root, ["--rnd_resized", "4"])
    data = os.path.join(root, "data", "synthetic_tiny_imagenet")
    assert sorted(f for f in os.listdir(data) if f.endswith(".pth.tar")) == ["task_1_rndtrans.pth.tar", "task_2_rndtrans.pth.tar"]
    t1 = torch.load(os.path.join(data, "task_1_rndtrans.pth.tar"), weights_only=False)
    assert isinstance(t1["train"].transform, RandomResizedCropFlip) and tuple(t1["train"].x.shape[1:]) == (3, 36, 36)
    assert t1["test"].transform is None and tuple(t1["test"].x.shape[1:]) == (3, 32, 32)
    res = out["results"]
    assert sorted(res) == [0, 1] and len(res[0]["seq_res"][0]) == 2 and len(res[1]["seq_res"][1]) == 1
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("EWC on resampled tasks:", accs)
    assert _finite(accs)
    tdir = os.path.join(out["manager"].parent_exp_dir, "task_2", "TASK_TRAINING")
    assert os.path.exists(os.path.join(tdir, "SUCCESS.FLAG")) and os.path.exists(os.path.join(tdir, "best_model.pth.tar"))


def test_joint_through_the_driver_on_resampled_tasks(tmp_path):
    from clsurvey_amd.framework import driver
    root = str(tmp_path)
    _friendly_base_model(root)
    out = driver.main(_common(root, ["--rnd_resized", "4"]) + ["--method_name", "joint", "--test"])
    assert all(os.path.basename(p).endswith("_rndtrans.pth.tar") for p in out["ds_paths"]) and len(out["ds_paths"]) == 2
    accs = out["results"]["joint"]["seq_res"]
    print("joint on resampled tasks:", accs)
    assert len(accs) == 2 and _finite(accs)
    assert os.path.exists(out["model_paths"][0]) and os.listdir(out["args"].out_path)


def test_rnd_resized_zero_is_a_run_without_the_flag(tmp_path):
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    _ewc(a, ["--rnd_resized", "0"])
    _ewc(b, [])
    fa, fb = _model_files(a), _model_files(b)
    assert len(fa) >= 2 and sorted(fa) == sorted(fb)
    for name in fa:
        assert fa[name] == fb[name], name
    names = sorted(os.listdir(os.path.join(a, "data", "synthetic_tiny_imagenet")))
    assert names == sorted(os.listdir(os.path.join(b, "data", "synthetic_tiny_imagenet"))) and not any("rndtrans" in n for n in names)


def test_rnd_resized_and_rnd_margin_exclude_each_other(tmp_path):
    from clsurvey_amd.framework import driver
    with pytest.raises(SystemExit):
        driver.main(_common(str(tmp_path), ["--rnd_resized", "4", "--rnd_margin", "4"]) + ["--method_name", "EWC"])
