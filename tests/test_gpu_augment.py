"""On-device crop + flip augmentation on the GPU: clhip_gather_tasks_crop_flip against four lines of torch slicing (a copy:
bitwise, no tolerance), its safety rule, the augmented loaders against (order, draw_crop_flip(base seed)) recomputed on the
host, a transform without freedom as the identity of a training epoch, and `--rnd_margin` through the driver."""
import os
from itertools import accumulate

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def restate(frames, idx, params, th, tw):
    """torchvision's crop, then hflip, of frames[idx[b]] with params[b] = (top, left, flip), on the CPU."""
    rows = [frames[g, :, top:top + th, left:left + tw] for g, (top, left, _) in zip(idx.tolist(), params.tolist())]
    return torch.stack([v.flip(-1) if flip else v for v, (_, _, flip) in zip(rows, params.tolist())])


def _tasks(C, Hs, Ws, seed):
    gen = torch.Generator().manual_seed(seed)
    sizes, ncls = [5, 1, 7], [3, 2, 4]
    xs = [torch.randn((n, C, Hs, Ws), generator=gen) for n in sizes]
    ys = [torch.randint(0, k, (n,), generator=gen) for n, k in zip(sizes, ncls)]
    shifts = [0] + list(accumulate(ncls))[:-1]
    return xs, ys, list(accumulate(sizes)), shifts


def _table(xs, ys, cum, shifts):
    from clsurvey_amd import ops
    dev_x, dev_y = [x.to(DEV) for x in xs], [y.to(DEV) for y in ys]
    return ops.task_table(dev_x, dev_y, cum, shifts, DEV), (dev_x, dev_y)          # (the table holds pointers: keep the tensors)


GEOMETRIES = [(13, 11, 8, 7), (20, 20, 16, 16), (16, 16, 16, 16), (9, 40, 9, 1), (40, 72, 36, 64), (40, 72, 36, 63), (72, 72, 70, 64),
              (5, 4200, 2, 4100)]


@pytest.mark.parametrize("Hs,Ws,th,tw", GEOMETRIES, ids=["%dx%d_to_%dx%d" % g for g in GEOMETRIES])
def test_kernel_is_bitwise_crop_then_flip(Hs, Ws, th, tw):
    """T = 3 tasks of 5 / 1 / 7 frames, B = 9 across every task boundary, sample 4 twice with two parameter rows; offsets 0 and
    the maximum in both axes, mixed flips.  odd widths (no vector path) / vector stores with odd left / no freedom / one column /
    a row above one block's segment / the same on the plain path (several rounds per thread) / more than one chunk of lines per
    channel with a short last chunk / a line longer than a block's segment."""
    from clsurvey_amd import ops
    xs, ys, cum, shifts = _tasks(3, Hs, Ws, 100 + Hs + tw)
    table, keep = _table(xs, ys, cum, shifts)
    mt, ml = Hs - th, Ws - tw
    idx = torch.tensor([0, 4, 5, 6, 12, 4, 9, 5, 11])
    params = torch.tensor([[0, 0, 0], [mt, ml, 1], [0, ml, 1], [mt, 0, 0], [mt, ml, 0], [mt // 2, min(1, ml), 0],
                           [min(1, mt), ml // 2, 1], [mt, min(3, ml), 1], [0, 0, 1]], dtype=torch.int32)
    x, y = ops.gather_tasks_crop_flip(table, (3, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV))
    assert tuple(x.shape) == (9, 3, th, tw) and x.dtype == torch.float32
    want = restate(torch.cat(xs), idx, params, th, tw)
    assert torch.equal(x.cpu(), want)
    assert torch.equal(y.cpu(), torch.cat([v + s for v, s in zip(ys, shifts)])[idx])
    if ml and mt:
        assert not torch.equal(x[1], x[5])                                         # one sample, two parameter rows


def test_unaligned_output_takes_the_plain_path():
    """tw % 4 == 0 but x_out 4 bytes off a 16-byte boundary: no vector stores, same bytes."""
    from clsurvey_amd import ops
    xs, ys, cum, shifts = _tasks(3, 20, 20, 7)
    table, keep = _table(xs, ys, cum, shifts)
    idx = torch.tensor([12, 0, 5])
    params = torch.tensor([[4, 3, 1], [0, 0, 0], [1, 4, 1]], dtype=torch.int32)
    buf = torch.full((1 + 3 * 3 * 16 * 16,), -7.0, device=DEV)
    assert buf[1:].data_ptr() % 16 == 4
    x, _ = ops.gather_tasks_crop_flip(table, (3, 20, 20, 16, 16), idx.to(DEV), params.to(DEV), x_out=buf[1:])
    assert torch.equal(x.cpu().view(3, 3, 16, 16), restate(torch.cat(xs), idx, params, 16, 16)) and float(buf[0]) == -7.0


def test_bad_rows_copy_nothing_and_get_label_minus_one():
    """The kernel's defined behaviour for a table the host would never upload: sample number == total, -1, top one past its
    range, flip = 2 (and left / top below 0), between good rows.  Those rows keep the sentinel; the good ones are exact."""
    from clsurvey_amd import ops
    Hs, Ws, th, tw = 20, 20, 16, 16
    xs, ys, cum, shifts = _tasks(3, Hs, Ws, 5)
    table, keep = _table(xs, ys, cum, shifts)
    idx = torch.tensor([3, 13, 6, -1, 5, 2, 12, 7, 1])
    params = torch.tensor([[1, 2, 1], [0, 0, 0], [4, 4, 0], [0, 0, 0], [Hs - th + 1, 0, 0], [2, 2, 2], [0, 3, 1], [0, -1, 0],
                           [-1, 0, 1]], dtype=torch.int32)
    bad = [1, 3, 4, 5, 7, 8]
    good = [0, 2, 6]
    x = torch.full((9, 3, th, tw), -7.0, device=DEV)
    labels = torch.full((9,), 99, dtype=torch.int64, device=DEV)
    ops.gather_tasks_crop_flip(table, (3, Hs, Ws, th, tw), idx.to(DEV), params.to(DEV), x_out=x, labels_out=labels)
    x, labels = x.cpu(), labels.cpu()
    assert bool((x[bad] == -7.0).all()) and labels[bad].tolist() == [-1] * len(bad)
    assert torch.equal(x[good], restate(torch.cat(xs), idx[good], params[good], th, tw))
    assert torch.equal(labels[good], torch.cat([v + s for v, s in zip(ys, shifts)])[idx[good]])


def test_a_batch_larger_than_one_launch_goes_in_pieces():
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(4)
    xs, ys, cum, shifts = _tasks(1, 2, 3, 8)
    table, keep = _table(xs, ys, cum, shifts)
    B = 70000
    idx = torch.randint(0, 13, (B,), generator=gen)
    params = torch.stack([torch.randint(0, 2, (B,), generator=gen) for _ in range(3)], 1).to(torch.int32)
    x, y = ops.gather_tasks_crop_flip(table, (1, 2, 3, 1, 2), idx.to(DEV), params.to(DEV))
    frames = torch.cat(xs)
    rows = frames[idx, 0, params[:, 0].long()]                                     # [B, 3]: the line each position reads
    left = params[:, 1].long()
    a, b = rows.gather(1, left[:, None]), rows.gather(1, left[:, None] + 1)
    want = torch.where(params[:, 2:3] == 1, torch.cat([b, a], 1), torch.cat([a, b], 1))
    assert torch.equal(x.cpu().view(B, 2), want)
    assert torch.equal(y.cpu(), torch.cat([v + s for v, s in zip(ys, shifts)])[idx])


# ---------------------------------------------------------------------------------------------- loaders
def _sequence(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                               name="aug2", rnd_margin=4, **kw)
    return ds, [ds.get_task_dataset_path(str(t), rnd_transform=True) for t in (1, 2)]


def _host_epoch(n, shuffle, spec, frame_hw):
    """What an augmented loader does with the global generator and its base seed, restated: (order, parameter table)."""
    from clsurvey_amd.data import draw_crop_flip
    base = int(torch.empty((), dtype=torch.int64).random_().item())
    perm = None
    if shuffle:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = draw_crop_flip(n, spec, frame_hw, torch.Generator().manual_seed(base), order=perm)
    return (torch.arange(n) if perm is None else perm), table


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "in_order"])
@pytest.mark.parametrize("multi", [False, True], ids=["DeviceLoader", "MultiTaskLoader"])
def test_loader_serves_the_restatement_of_its_own_draws(tmp_path, multi, shuffle):
    from clsurvey_amd.data import DeviceLoader, MultiTaskLoader, RandomCropFlip, TaskList, load_task_datasets
    _, paths = _sequence(str(tmp_path))
    tasks = [load_task_datasets(p, DEV)["train"] for p in paths]
    assert all(isinstance(t.transform, RandomCropFlip) and t.x.is_cuda and tuple(t.x.shape) == (24, 3, 20, 20) for t in tasks)
    if multi:
        loader = MultiTaskLoader(TaskList(tasks), 7, shuffle, DEV)
        frames = torch.cat([t.x for t in tasks]).cpu()
        labels = torch.cat([t.y + s for t, s in zip(tasks, (0, 4))]).cpu()
    else:
        loader = DeviceLoader(tasks[0], 7, shuffle, DEV)
        frames, labels = tasks[0].x.cpu(), tasks[0].y.cpu()
    n = frames.shape[0]
    assert tuple(loader.x.shape) == (0, 3, 16, 16) and tuple(loader.x.shape[1:]) == (3, 16, 16) and len(loader) == (n + 6) // 7
    torch.manual_seed(3)
    got = list(loader)
    after = torch.get_rng_state()
    torch.manual_seed(3)
    order, table = _host_epoch(n, shuffle, tasks[0].transform, (20, 20))
    assert torch.equal(after, torch.get_rng_state())
    assert [b[0].shape[0] for b in got] == [7] * (n // 7) + ([n % 7] if n % 7 else [])
    assert torch.equal(torch.cat([b[0] for b in got]).cpu(), restate(frames, order, table, 16, 16))
    assert torch.equal(torch.cat([b[1] for b in got]).cpu(), labels[order])
    assert len(set(map(tuple, table.tolist()))) > 5                                 # the draws do differ between positions
    # the next epoch serves the same samples under other crops
    second = list(loader)
    if not shuffle:
        a, b = torch.cat([v[0] for v in got]), torch.cat([v[0] for v in second])
        assert torch.equal(torch.cat([v[1] for v in second]).cpu(), labels) and not torch.equal(a, b)
        assert sum(int(not torch.equal(a[i], b[i])) for i in range(n)) > n // 2


def test_a_plain_and_an_augmented_loader_serve_the_same_samples(tmp_path):
    """Same RNG state, same sample order: the labels agree batch by batch, and each served image is a 16 x 16 window of the
    frame whose centre crop the plain loader serves."""
    from clsurvey_amd.data import DeviceLoader, load_task_datasets
    ds, paths = _sequence(str(tmp_path))
    aug = load_task_datasets(paths[0], DEV)["train"]
    raw = load_task_datasets(ds.get_task_dataset_path("1"), DEV)["train"]
    assert raw.transform is None
    torch.manual_seed(11)
    a = list(DeviceLoader(aug, 7, True, DEV))
    torch.manual_seed(11)
    b = list(DeviceLoader(raw, 7, True, DEV))
    assert len(a) == len(b) == 4
    for (xa, ya), (xb, yb) in zip(a, b):
        assert xa.shape == xb.shape and torch.equal(ya, yb)


def test_transform_without_freedom_is_the_identity_of_a_training_epoch(tmp_path):
    """size == frame and p = 0: the augmented path changes nothing but the pixels, and here not those — one epoch of
    fine_tune_SGD leaves the parameters bitwise equal to the same epoch through the plain loader."""
    from clsurvey_amd import models
    from clsurvey_amd.data import DeviceLoader, RandomCropFlip, TensorTaskDataset, load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import finetune
    root = str(tmp_path)
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=1, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="mem1")
    dsets = load_task_datasets(ds.get_task_dataset_path("1"), DEV)
    torch.manual_seed(0)
    base = os.path.join(root, "base.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), base)
    params = []
    for tag in ("augmented", "plain"):
        spec = RandomCropFlip((32, 32), p=0.0) if tag == "augmented" else None
        per = {s: TensorTaskDataset(dsets[s].x, dsets[s].y, dsets[s].classes, transform=spec) for s in ("train", "val")}
        torch.manual_seed(7)
        loaders = {s: DeviceLoader(per[s], 40, True, DEV) for s in per}
        assert (loaders["train"].transform is not None) == (tag == "augmented") and tuple(loaders["train"].x.shape[1:]) == (3, 32, 32)
        model, _ = finetune.fine_tune_SGD(loaders, {s: len(per[s]) for s in per}, {s: [per[s].classes] for s in per},
                                          model_path=base, exp_dir=os.path.join(root, tag), num_epochs=1, lr=1e-2, device=DEV,
                                          batch_size=40)
        params.append([p.detach().clone() for p in model.parameters()])
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


def test_ewc_through_the_driver_on_augmented_tasks(tmp_path):
    """SI dump, LR grid, a Fisher pass over an augmented reg_sets loader, evaluation on the static test split."""
    from clsurvey_amd.data import RandomCropFlip
    root = str(tmp_path)
    out = _ewc(root, ["--rnd_margin", "4"])
    data = os.path.join(root, "data", "synthetic_tiny_imagenet")
    assert sorted(f for f in os.listdir(data) if f.endswith(".pth.tar")) == ["task_1_rndtrans.pth.tar", "task_2_rndtrans.pth.tar"]
    t1 = torch.load(os.path.join(data, "task_1_rndtrans.pth.tar"), weights_only=False)
    assert isinstance(t1["train"].transform, RandomCropFlip) and tuple(t1["train"].x.shape[1:]) == (3, 36, 36)
    assert t1["test"].transform is None and tuple(t1["test"].x.shape[1:]) == (3, 32, 32)
    res = out["results"]
    assert sorted(res) == [0, 1] and len(res[0]["seq_res"][0]) == 2 and len(res[1]["seq_res"][1]) == 1
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("EWC on augmented tasks:", accs)
    assert _finite(accs)
    tdir = os.path.join(out["manager"].parent_exp_dir, "task_2", "TASK_TRAINING")
    assert os.path.exists(os.path.join(tdir, "SUCCESS.FLAG")) and os.path.exists(os.path.join(tdir, "best_model.pth.tar"))
    om = torch.load(os.path.join(tdir, "best_model.pth.tar"), weights_only=False).reg_params
    assert any(float(v["omega"].abs().max()) > 0 for k, v in om.items() if isinstance(v, dict) and "omega" in v)
    assert os.listdir(out["args"].out_path)


def test_joint_through_the_driver_on_augmented_tasks(tmp_path):
    from clsurvey_amd.framework import driver
    root = str(tmp_path)
    _friendly_base_model(root)
    out = driver.main(_common(root, ["--rnd_margin", "4"]) + ["--method_name", "joint", "--test"])
    assert all(os.path.basename(p).endswith("_rndtrans.pth.tar") for p in out["ds_paths"]) and len(out["ds_paths"]) == 2
    accs = out["results"]["joint"]["seq_res"]
    print("joint on augmented tasks:", accs)
    assert len(accs) == 2 and _finite(accs)
    assert os.path.exists(out["model_paths"][0]) and os.listdir(out["args"].out_path)


def test_margin_zero_is_a_run_without_the_flag(tmp_path):
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    _ewc(a, ["--rnd_margin", "0"])
    _ewc(b, [])
    fa, fb = _model_files(a), _model_files(b)
    assert len(fa) >= 2 and sorted(fa) == sorted(fb)
    for name in fa:
        assert fa[name] == fb[name], name
    names = sorted(os.listdir(os.path.join(a, "data", "synthetic_tiny_imagenet")))
    assert names == sorted(os.listdir(os.path.join(b, "data", "synthetic_tiny_imagenet"))) and not any("rndtrans" in n for n in names)


def test_margin_needs_the_synthetic_sequence(tmp_path):
    from clsurvey_amd.framework import driver
    with pytest.raises(SystemExit):
        driver.main(["small_VGG9_cl_128_128", "--method_name", "EWC", "--results_root", str(tmp_path), "--rnd_margin", "4"])
