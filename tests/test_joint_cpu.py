"""Joint baseline without a GPU — fixture G36 (tests/golden/make_g36.py: recorded from the reference's own
methods/method.py:1185-1235 and framework/eval.py:69-143): the method row, its hooks, the phase-1 argument map, the
single-model evaluation loop scenario by scenario, the index arithmetic of the multi-task loader and the argument checks of
the two ABI entries."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g36_common as G  # noqa: E402


@pytest.fixture(scope="module")
def g36():
    with open(os.path.join(HERE, "golden", "G36_joint.json")) as f:
        return json.load(f)


def _json(v):
    return json.loads(json.dumps(v))


def test_joint_row_matches_reference_g36(g36):
    from clsurvey_amd.methods import method as M
    m = M.parse("joint")
    assert isinstance(m, M.Joint) and _json(G.describe(m)) == g36["row"]
    assert G.get_output_error(m) == g36["get_output_raises"]
    with pytest.raises(NotImplementedError):
        m.get_output(torch.zeros(1), None)
    assert m.train is None                                  # grid only: no phase 2


def test_joint_hooks_match_reference_g36(g36):
    from clsurvey_amd.methods import finetune, method as M
    assert _json(G.hooks(M.parse("joint"))) == g36["hooks"]
    assert _json(G.phase1_call(M.parse("joint"), finetune)) == g36["phase1_call"]


def test_synthetic_sequence_has_no_joint_file(tmp_path):
    from types import SimpleNamespace
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import method as M
    ds = SyntheticTaskSequence(str(tmp_path), task_count=3, classes_per_task=2, sizes=(4, 2, 2), hw=8, name="s")
    assert ds.get_task_dataset_path(task_name=None, rnd_transform=True) is None
    paths = M.parse("joint").grid_datafetch(SimpleNamespace(task_name="1"), ds)
    assert paths == [ds.get_task_dataset_path(str(t)) for t in (1, 2, 3)] and all(os.path.exists(p) for p in paths)


@pytest.mark.parametrize("case", range(len(G.SINGLE_CASES)), ids=[c["tag"] for c in G.SINGLE_CASES])
def test_eval_single_model_all_tasks_g36(g36, case):
    from clsurvey_amd.framework import driver
    keep, G.SINGLE_CASES = G.SINGLE_CASES, [G.SINGLE_CASES[case]]
    try:
        got = G.single_evals(driver.eval_single_model_all_tasks,
                             lambda name: driver.get_perf_output_filename(name, None, joint_full_batch=True))
    finally:
        G.SINGLE_CASES = keep
    assert _json(got[0]) == g36["single_evals"][case]


def _uneven_tasks():
    from clsurvey_amd.data import TensorTaskDataset
    gen = torch.Generator().manual_seed(5)
    out = []
    for n, k in ((7, 3), (1, 2), (12, 4), (5, 1)):
        out.append(TensorTaskDataset(torch.randn((n, 2, 3), generator=gen), torch.randint(0, k, (n,), generator=gen),
                                     [str(c) for c in range(k)]))
    return out


def test_task_list_index_arithmetic_equals_concat_tasks():
    from clsurvey_amd.data import TaskList
    from clsurvey_amd.methods.method import ConcatTasks
    dsets = _uneven_tasks()
    merged = ConcatTasks(dsets, [len(d.classes) for d in dsets])
    tl = TaskList(dsets)
    assert len(tl) == len(merged) == 25 and tl.classes == merged.classes
    assert tl.cumulative_classes_len == [3, 5, 9, 10] and tl.cumulative_sizes == [7, 8, 20, 25]
    idx = torch.randperm(len(tl), generator=torch.Generator().manual_seed(1))
    task, row, shift = tl.locate(idx)
    for g, t, r, s in zip(idx.tolist(), task.tolist(), row.tolist(), shift.tolist()):
        assert torch.equal(dsets[t].x[r], merged.x[g]) and int(dsets[t].y[r]) + s == int(merged.y[g])
        x, y = tl[g]
        assert torch.equal(x, merged.x[g]) and int(y) == int(merged.y[g])
    for bad in (-1, 25):
        with pytest.raises(IndexError):
            tl.locate([bad])


@pytest.mark.parametrize("shuffle", [True, False])
def test_multi_task_loader_pass_equals_device_loader_pass(monkeypatch, shuffle):
    """MultiTaskLoader's own constructor and __iter__, with the two device calls replaced by host stand-ins that do what the
    header says: a whole pass yields DeviceLoader's batches over the merged copy and leaves the global generator in the same
    state (nothing but order() may draw from it)."""
    from clsurvey_amd import ops
    from clsurvey_amd.data import DeviceLoader, MultiTaskLoader, TaskList
    from clsurvey_amd.methods.method import ConcatTasks
    dsets = _uneven_tasks()

    def task_table(xs, ys, cum_rows, label_shifts, device):
        return list(zip(xs, ys, cum_rows, label_shifts))

    def gather_tasks(table, row_elems, idx):
        rows, labels = [], []
        for g in idx.tolist():
            t = next(j for j, (_, _, cum, _) in enumerate(table) if cum > g)      # first task whose cumulative count exceeds g
            x, y, _, shift = table[t]
            local = g - (table[t - 1][2] if t else 0)
            rows.append(x[local].reshape(-1))
            labels.append(int(y[local]) + shift)
        return torch.stack(rows), torch.tensor(labels, dtype=torch.int64)

    monkeypatch.setattr(ops, "task_table", task_table)
    monkeypatch.setattr(ops, "gather_tasks", gather_tasks)
    ref = DeviceLoader(ConcatTasks(dsets, [len(d.classes) for d in dsets]), 4, shuffle, "cpu")
    new = MultiTaskLoader(TaskList(dsets), 4, shuffle, "cpu")
    assert len(new) == len(ref) == 7 and new.row_elems == 6 and tuple(new.x.shape) == (0, 2, 3)
    torch.manual_seed(11)
    a, s_ref = list(ref), torch.get_rng_state()
    torch.manual_seed(11)
    b, s_new = list(new), torch.get_rng_state()
    assert torch.equal(s_ref, s_new) and len(a) == len(b) == 7
    for (xa, ya), (xb, yb) in zip(a, b):
        assert xa.shape == xb.shape and torch.equal(xa, xb) and torch.equal(ya, yb)


def test_joint_abi_entries_reject_bad_arguments():
    import ctypes as C
    from clsurvey_amd import _lib
    L = _lib.lib()
    one = C.c_void_p(16)                                    # never dereferenced: every call below stops at the checks
    assert L.clhip_gather_tasks(None, 3, 16, one, 4, one, one, None) == -1
    assert L.clhip_gather_tasks(one, 0, 16, one, 4, one, one, None) == -1
    assert L.clhip_gather_tasks(one, 65, 16, one, 4, one, one, None) == -1
    assert L.clhip_gather_tasks(one, 3, 0, one, 4, one, one, None) == -1
    assert L.clhip_gather_tasks(one, 3, 16, None, 4, one, one, None) == -1
    assert L.clhip_gather_tasks(one, 3, 16, one, 70000, one, one, None) == -1
    assert L.clhip_gather_tasks(one, 3, 16, one, 0, one, one, None) == 0       # nothing to do
    assert L.clhip_slice_argmax_count(None, 4, 8, one, 4, one, one, one, one, None) == -1
    assert L.clhip_slice_argmax_count(one, 4, 8, one, 9, one, one, one, one, None) == -1       # K > ld
    assert L.clhip_slice_argmax_count(one, 4, 8, one, 0, one, one, one, one, None) == -1
    assert L.clhip_slice_argmax_count(one, -1, 8, one, 4, one, one, one, one, None) == -1
    assert L.clhip_slice_argmax_count(one, 4, 8, one, 4, one, one, one, None, None) == -1
    assert "clhip_gather_tasks" in _lib.SIGNATURES and "clhip_slice_argmax_count" in _lib.SIGNATURES


def test_shard_test_is_refused_for_joint(tmp_path):
    from clsurvey_amd.framework import driver
    with pytest.raises(SystemExit, match="joint"):
        driver.main(["small_VGG9_cl_128_128", "--method_name", "joint", "--shard", "--test", "--results_root", str(tmp_path)])
