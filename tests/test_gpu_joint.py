"""Joint baseline on the GPU: the two kernels of csrc/joint.hip against torch, the multi-task loader against the merged-copy
path it replaces, and the evaluation / the whole `--method_name joint --test` run against fixture G36 (recorded from the
reference's unchanged framework/main.py, tests/golden/make_g36.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g36_common as G  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def g36():
    with open(os.path.join(HERE, "golden", "G36_joint.json")) as f:
        data = json.load(f)
    arrays = {}
    for name in ("G36_joint.npz", "G36_joint_part2.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as z:
            arrays.update({k: z[k] for k in z.files})
    return data, arrays


# ---------------------------------------------------------------------------------------------- clhip_gather_tasks
def _sources(T, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    sizes = [1 + (5 * j + 3) % 11 for j in range(T)]                       # uneven, some tasks of a single row
    ncls = [1 + j % 4 for j in range(T)]
    xs = [torch.randn((n,) + shape, generator=gen).to(DEV) for n in sizes]
    ys = [torch.randint(0, k, (n,), generator=gen).to(DEV) for n, k in zip(sizes, ncls)]
    return xs, ys, sizes, ncls


@pytest.mark.parametrize("shape", [(3, 64, 64), (3, 32, 32), (5, 3)], ids=["3x64x64", "3x32x32", "15_scalar_path"])
@pytest.mark.parametrize("T", [1, 3, 10])
def test_gather_tasks_is_bitwise_index_select_of_the_concatenation(T, shape):
    from itertools import accumulate
    from clsurvey_amd import ops
    xs, ys, sizes, ncls = _sources(T, shape, 100 + T)
    cum = list(accumulate(sizes))
    shifts = [0] + list(accumulate(ncls))[:-1]
    table = ops.task_table(xs, ys, cum, shifts, DEV)
    merged_x = torch.cat(xs).flatten(1)
    merged_y = torch.cat([y + s for y, s in zip(ys, shifts)])
    row_elems = merged_x.shape[1]
    edges = sorted({0} | {c - 1 for c in cum} | {c for c in cum[:-1]})       # first and last row of every task
    gen = torch.Generator().manual_seed(T)
    for B in (1, 40, 200):
        for idx in (torch.randint(0, cum[-1], (B,), generator=gen), torch.tensor((edges * B)[:B])):
            idx = idx.to(DEV)
            x, y = ops.gather_tasks(table, row_elems, idx)
            assert torch.equal(x, merged_x.index_select(0, idx)), (T, shape, B)
            assert torch.equal(y, merged_y.index_select(0, idx)), (T, shape, B)
    idx = torch.tensor(edges).to(DEV)                                          # every boundary row in one batch
    x, y = ops.gather_tasks(table, row_elems, idx)
    assert torch.equal(x, merged_x.index_select(0, idx)) and torch.equal(y, merged_y.index_select(0, idx))


def test_gather_tasks_takes_a_batch_larger_than_one_launch():
    """One launch takes 65535 rows; ops.gather_tasks issues a larger batch in pieces."""
    from itertools import accumulate
    from clsurvey_amd import ops
    xs, ys, sizes, ncls = _sources(3, (4,), 9)
    cum = list(accumulate(sizes))
    shifts = [0] + list(accumulate(ncls))[:-1]
    table = ops.task_table(xs, ys, cum, shifts, DEV)
    idx = torch.randint(0, cum[-1], (70000,), generator=torch.Generator().manual_seed(2)).to(DEV)
    x, y = ops.gather_tasks(table, 4, idx)
    assert torch.equal(x, torch.cat(xs).index_select(0, idx))
    assert torch.equal(y, torch.cat([v + s for v, s in zip(ys, shifts)]).index_select(0, idx))


def test_loader_rejects_a_sample_number_outside_the_sequence_on_the_host():
    from clsurvey_amd.data import MultiTaskLoader, TaskList, TensorTaskDataset
    d = [TensorTaskDataset(torch.zeros(3, 4).to(DEV), torch.zeros(3, dtype=torch.int64).to(DEV), ["a"]) for _ in range(2)]
    loader = MultiTaskLoader(TaskList(d), 4, True, DEV)
    loader.order = lambda: torch.tensor([0, 5, 6, 1])
    with pytest.raises(IndexError):
        next(iter(loader))


def _sequence(root, sizes=(400, 40, 40)):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=3, classes_per_task=4, sizes=sizes, hw=32, noise=0.4,
                               name="mem3")
    return ds, [ds.get_task_dataset_path(str(t)) for t in (1, 2, 3)]


def test_joint_loader_makes_no_merged_copy(tmp_path):
    """Tasks already in the cache: the joint loader allocates less than ONE task's images, the merged-copy path all of them."""
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.methods import method as M
    _, paths = _sequence(str(tmp_path))
    tasks = [load_task_datasets(p, DEV) for p in paths]
    one_task = tasks[0]["train"].x.numel() * 4
    all_tasks = sum(t[s].x.numel() * 4 for t in tasks for s in ("train", "val"))
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    joint = M.compose_joint_dataset(paths, 40, DEV)
    m1 = torch.cuda.memory_allocated()
    merged = M.compose_dataset(paths, 40, DEV)
    m2 = torch.cuda.memory_allocated()
    print("joint loader: +%d B, merged copy: +%d B (one task %d B, all %d B)" % (m1 - m0, m2 - m1, one_task, all_tasks))
    assert m1 - m0 < one_task
    assert m2 - m1 >= all_tasks
    assert joint[1] == merged[1] and joint[2] == merged[2]
    assert joint[0]["train"].dataset.cumulative_classes_len == [4, 8, 12]


def test_joint_loader_yields_the_batches_of_the_merged_copy(tmp_path):
    from clsurvey_amd.methods import method as M
    _, paths = _sequence(str(tmp_path), sizes=(50, 7, 7))
    joint, merged = M.compose_joint_dataset(paths, 40, DEV)[0], M.compose_dataset(paths, 40, DEV)[0]
    for split in ("train", "val"):
        torch.manual_seed(3)
        a = list(joint[split])
        torch.manual_seed(3)
        b = list(merged[split])
        assert len(a) == len(b) == len(joint[split]) == len(merged[split])
        for (xa, ya), (xb, yb) in zip(a, b):
            assert xa.shape == xb.shape and torch.equal(xa, xb) and torch.equal(ya, yb)


def test_one_joint_epoch_equals_the_merged_copy_epoch_bitwise(tmp_path):
    """The loader changes where batches come from, not what they are: same seed, same parameters after one epoch."""
    from clsurvey_amd import models
    from clsurvey_amd.methods import finetune, method as M
    root = str(tmp_path)
    _, paths = _sequence(root, sizes=(80, 20, 20))
    torch.manual_seed(0)
    base = os.path.join(root, "base.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), base)
    params = []
    for tag, compose in (("joint", M.compose_joint_dataset), ("merged", M.compose_dataset)):
        torch.manual_seed(7)
        loaders, sizes, classes = compose(paths, 40, DEV)
        model, _ = finetune.fine_tune_SGD(loaders, sizes, classes, model_path=base, exp_dir=os.path.join(root, tag), num_epochs=1,
                                          lr=1e-2, device=DEV, batch_size=40)
        params.append([p.detach().clone() for p in model.parameters()])
    assert params[0][-1].shape[0] == 12
    for a, b in zip(*params):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- clhip_slice_argmax_count
def _reference_counts(logits, cols, labels, K):
    """framework/inference.py:141-149 on the CPU; rows whose label is outside [0, K) are counted apart."""
    inside = logits[:, cols]
    _, predicted = torch.max(inside, 1)
    correct, total, bad = torch.zeros(K, dtype=torch.int64), torch.zeros(K, dtype=torch.int64), 0
    for i in range(len(predicted)):
        label = int(labels[i])
        if not 0 <= label < K:
            bad += 1
            continue
        correct[label] += int(predicted[i] == label)
        total[label] += 1
    return correct, total, bad


@pytest.mark.parametrize("scattered", [False, True], ids=["contiguous", "scattered"])
@pytest.mark.parametrize("N", [1, 40, 200])
@pytest.mark.parametrize("K", [1, 4, 20, 200])
def test_slice_argmax_count_equals_torch(K, N, scattered):
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(1000 * K + N)
    ld = 2 * K + 5
    cols = torch.randperm(ld, generator=gen)[:K].tolist() if scattered else list(range(3, 3 + K))
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(DEV)
    counters = torch.zeros(2 * K + 1, dtype=torch.int64, device=DEV)
    want_c, want_t, want_bad = torch.zeros(K, dtype=torch.int64), torch.zeros(K, dtype=torch.int64), 0
    for call in range(3):                                       # counters accumulate over calls
        logits = torch.randn((N, ld), generator=gen)
        labels = torch.randint(0, K, (N,), generator=gen)
        if K > 1:
            for i in range(0, N, 3):                            # exact ties between the maximum and another position
                a, b = torch.randperm(K, generator=gen)[:2].tolist()
                logits[i, cols[a]] = logits[i, cols[b]] = float(logits[i].max()) + 1.0
            for i in range(1, N, 7):                            # a NaN inside the slice, and one outside it
                logits[i, cols[int(torch.randint(0, K, (1,), generator=gen))]] = float("nan")
            if call == 1 and N > 2:
                logits[2, cols[0]] = logits[2, cols[K - 1]] = float("nan")
        outside = [c for c in range(ld) if c not in cols]
        logits[0, outside[0]] = float("nan") if call == 0 else 1e9
        if call == 2:
            labels[0] = K                                       # out of range: counted apart, the other rows still count
            if N > 5:
                labels[5] = -1
        c, t, bad = _reference_counts(logits, cols, labels, K)
        want_c, want_t, want_bad = want_c + c, want_t + t, want_bad + bad
        ops.slice_argmax_count(logits.to(DEV), cols_dev, labels.to(DEV), counters[:K], counters[K:2 * K], counters[2 * K:])
    got = counters.cpu()
    assert torch.equal(got[:K], want_c) and torch.equal(got[K:2 * K], want_t) and int(got[2 * K]) == want_bad
    assert want_bad >= 1 and int(want_t.sum()) + want_bad == 3 * N


def test_evaluation_raises_on_a_label_outside_the_slice(tmp_path):
    from clsurvey_amd import models
    from clsurvey_amd.framework import inference
    _, paths = _sequence(str(tmp_path), sizes=(8, 8, 40))
    path = os.path.join(str(tmp_path), "m.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 12), path)
    with pytest.raises(IndexError):
        inference.test_task_joint_model(path, paths[0], 0, [2, 4, 4], batch_size=8, device=DEV)      # labels reach 3, slice has 2


# ---------------------------------------------------------------------------------------------- fixture G36
def _tiny3(root):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    return SyntheticTaskSequence(os.path.join(root, "data"), **G.TINY3)


def test_teacher_forced_evaluation_matches_reference_g36(g36, tmp_path):
    """The reference's winning joint model through the build's evaluation: logits within the G33 bound (1e-4 of the logit
    scale), seq_res and every per-class counter equal to the reference's.  Test images whose two largest in-slice logits are
    closer than that bound are listed in the fixture (at most 1 of 120; this fixture lists none) and would be exempt."""
    from types import SimpleNamespace
    from clsurvey_amd import models
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.framework import driver, inference
    from clsurvey_amd.methods import method as M
    from clsurvey_amd.net import NetEngine
    data, arr = g36
    root = str(tmp_path)
    ds = _tiny3(root)
    run = data["end_to_end"]["runs"][data["end_to_end"]["recorded_run"]]
    model = models.parse_model_name(G.MODEL, (32, 32), run["head_width"])
    plist = list(model.parameters())
    assert len(plist) == len([k for k in arr if k.startswith("p")]) == 18
    with torch.no_grad():
        for i, p in enumerate(plist):
            p.copy_(torch.from_numpy(arr["p%d" % i]))
    path = os.path.join(root, "best_model.pth.tar")
    torch.save(model, path)
    exempt = data["near_tie_test_images"]
    assert len(exempt) <= 1
    ref_seq = dict(dict(run["result"])["joint"])["seq_res"]

    ds_paths = [ds.get_task_dataset_path(str(t)) for t in (1, 2, 3)]
    engine = NetEngine(model.to(DEV).eval(), 40, (3, 32, 32), DEV)
    for t in range(3):
        x = load_task_datasets(ds_paths[t], DEV)["test"].x
        ref = torch.from_numpy(arr["logits_%d" % t])
        err = float((engine.forward(x).cpu() - ref).abs().max()) / float(ref.abs().max())
        print("task", t + 1, "logits error relative to the logit scale:", err)
        assert err <= 1e-4, (t, err)
        acc, correct, total = inference.test_task_joint_model(path, ds_paths[t], t, [4, 4, 4], batch_size=40, device=DEV,
                                                              tasks_idxes=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]],
                                                              per_class_stats=True)
        print("task", t + 1, "accuracy", acc, "reference", ref_seq[t], "correct", correct.tolist(), "total", total.tolist())
        slack = sum(1 for e in exempt if e[0] == t)
        assert torch.equal(total, torch.from_numpy(arr["total_%d" % t]))
        assert int((correct - torch.from_numpy(arr["correct_%d" % t])).abs().sum()) <= slack
        assert abs(acc - ref_seq[t]) <= 100.0 * slack / 40 + 1e-9
        # without tasks_idxes: the contiguous slice the class counts give (inference.py:124-125)
        assert inference.test_task_joint_model(path, ds_paths[t], t, [4, 4, 4], batch_size=40, device=DEV) == acc

    method = M.parse("joint")
    manager = driver.Manager(ds, method, path, root, None)
    args = SimpleNamespace(test_starting_task_count=1, test_max_task_count=3, batch_size=40, debug=False, device=DEV,
                           out_path=os.path.join(root, "test_out"), model_path=path, task_lengths=[4, 4, 4])
    res = driver.eval_single_model_all_tasks(args, manager, ds_paths)
    assert args.tasks_idxes == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    slack = [100.0 * sum(1 for e in exempt if e[0] == t) / 40 + 1e-9 for t in range(3)]
    assert all(abs(a - b) <= s for a, b, s in zip(res["joint"]["seq_res"], ref_seq, slack)), (res, ref_seq)
    saved = torch.load(os.path.join(args.out_path, run["result_file"]), weights_only=False)
    assert saved == res and os.listdir(args.out_path) == [run["result_file"]]


def test_joint_end_to_end_matches_reference_driver_g36(g36, tmp_path):
    """`--method_name joint --test` on tiny3 from the deterministic start weights, the flags of the reference's run: one task
    directory, a head of 12 outputs, the recorded winner, exp_name and result file; per-LR grid accuracy within two of the 120
    validation images and each task's test accuracy within three of its 40 test images (the rule of the G10 / G17 tests)."""
    from g10_weights import det_weights
    from clsurvey_amd import models
    from clsurvey_amd.framework import driver
    data, _ = g36
    run = data["end_to_end"]["runs"][data["end_to_end"]["recorded_run"]]
    root = str(tmp_path)
    ds = _tiny3(root)
    m = models.parse_model_name(G.MODEL, (32, 32), 4)
    with torch.no_grad():
        for p, w in zip(m.parameters(), det_weights()):
            p.copy_(torch.from_numpy(w))
    os.makedirs(os.path.join(root, "models"))
    torch.save(m, os.path.join(root, "models", G.MODEL + ".pth.tar"))
    assert data["end_to_end"]["argv"] == G.COMMON
    out = driver.main(G.COMMON + ["--method_name", "joint", "--results_root", root, "--test"], dataset=ds)
    mgr = out["manager"]
    assert out["args"].exp_name == run["exp_name"]
    assert sorted(os.listdir(mgr.parent_exp_dir)) == run["task_dirs"] == ["task_1"]
    assert len(out["ds_paths"]) == 3 and len(out["model_paths"]) == 1       # the one list of task files, unwrapped (eval.py:22)
    link = os.path.join(mgr.parent_exp_dir, "task_1", "TASK_TRAINING")
    assert os.path.islink(link) == run["task_training_is_link"]
    trace = {lr: acc for lr, it, acc in mgr.grid_trace}
    print("joint grid build:", trace, " reference:", run["grid"])
    assert os.path.basename(os.path.realpath(link)) == run["winner_dir"]
    two = 2.0 / 120 + 1e-9
    assert sorted(trace) == sorted(lr for lr, _ in run["grid"])
    for lr, acc in run["grid"]:
        assert abs(trace[lr] - acc[0]) <= two, (lr, trace[lr], acc)
    model = torch.load(out["model_paths"][0], weights_only=False)
    assert model.classifier[len(model.classifier) - 1].out_features == run["head_width"] == 12
    res = out["results"]
    ref = dict(run["result"])
    assert list(res) == list(ref) == ["joint"] and list(res["joint"]) == [k for k, _ in ref["joint"]] == ["seq_res"]
    out_dir = out["args"].out_path
    assert os.listdir(out_dir) == [run["result_file"]]
    assert torch.load(os.path.join(out_dir, run["result_file"]), weights_only=False) == res
    three = 100.0 * 3 / 40 + 1e-9
    ref_seq = dict(ref["joint"])["seq_res"]
    print("joint seq_res build:", res["joint"]["seq_res"], " reference:", ref_seq)
    assert len(res["joint"]["seq_res"]) == 3
    for a, b in zip(res["joint"]["seq_res"], ref_seq):
        assert abs(a - b) <= three, (res, ref_seq)
