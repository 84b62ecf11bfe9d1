"""Rehearsal baselines (R-PM / R-FM) without a GPU, against fixture G35 (tests/golden/make_g35.py): the method-table rows
and trainer arguments, main_rehearsal's batch split, the reference's exemplar draws, the memory counters and full-memory
truncation, and argument errors of the new ABI entries."""
import json
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g35_common as I  # noqa: E402


def _g35():
    with open(os.path.join(HERE, "golden", "G35_rehearsal_baselines.json")) as f:
        return json.load(f)


def test_method_rows_match_g35():
    from clsurvey_amd.methods import method as M
    ref = _g35()["methods"]
    for name, row in ref.items():
        m = M.parse(name)
        assert type(m).__name__ == row["class"]
        assert (m.name, m.eval_name, m.extra_hyperparams_count) == (row["name"], row["eval_name"], row["extra_hyperparams_count"])
        assert m.category.name == row["category"]
        assert list(m.hyperparams.items()) == [tuple(kv) for kv in row["hyperparams"]]
        assert getattr(m, "static_hyperparams", None) is None and row["static_hyperparams"] is None
        assert m.arg_string == row["arg_string"]
        for flag in ("start_scratch", "no_framework", "grid_chkpt", "wrap_first_task_model"):
            assert bool(getattr(m, flag, False)) == bool(row["flags"].get(flag, False)), (name, flag)
        for hook in row["hooks"]:
            assert callable(getattr(m, hook, None)), (name, hook)
        assert m.spec["output"] == "gem_slice" and m.spec["evaluate"] == "as_is"


def test_trainer_arguments_match_g35():
    """grid_train hands rehearsal main the reference's overwrite_args (method.py:1139-1165).  The reference reads
    manager.datasets (which Manager lacks) and args.mem_per_task (debug runmode only): the fixture's harness supplied both."""
    import contextlib
    import g28_common as G
    from clsurvey_amd.framework import driver
    from clsurvey_amd.methods import method as M
    ref = _g35()["hooks"]

    @contextlib.contextmanager
    def patches(log):
        saved = M._gem.main
        M._gem.main = G.Recorder(log, "rehearsal.main", None, (None, 0.5))
        try:
            yield
        finally:
            M._gem.main = saved
    saved = (G.METHODS, G.make_args)
    G.METHODS = list(I.NAMES)
    G.make_args = lambda task, _m=G.make_args: I.with_mem(_m(task))
    try:
        mine = json.loads(json.dumps(G.run(M.parse, driver.Manager, patches, set())))
    finally:
        G.METHODS, G.make_args = saved
    assert list(mine) == list(ref)
    for key in ref:
        a, b = mine[key], ref[key]
        assert a["ended"] == b["ended"], key
        assert [c["callee"] for c in a["calls"]] == [c["callee"] for c in b["calls"]], key
        for ca, cb in zip(a["calls"], b["calls"]):
            assert dict(map(tuple, ca["arguments"]["args"][0])) == dict(map(tuple, cb["arguments"]["args"][0])), key
            assert ca["arguments"]["args"][1:] == cb["arguments"]["args"][1:], key
        assert a["args"] == b["args"] and a["manager"] == b["manager"], key


def test_missing_mem_per_task_names_the_flag():
    from clsurvey_amd.methods import method as M
    m = M.parse("finetuning_rehearsal_partial_mem")
    args = types.SimpleNamespace(mem_per_task=None)
    with pytest.raises(ValueError, match="--mem_per_task"):
        m.grid_train(args, None, 0.01)
    from clsurvey_amd.framework import driver
    assert driver.build_parser().parse_args(["small_VGG9_cl_128_128"]).mem_per_task is None


def test_iCaRL_still_out_of_scope():
    from clsurvey_amd.methods import gem_main
    with pytest.raises(NotImplementedError):
        gem_main.main(dict(method="icarl", task_count=1, prev_model_path="x", n_tasks=1), [2])


def test_batch_split_matches_g35(monkeypatch, tmp_path):
    """main_rehearsal.py:181-202: loaders at the ORIGINAL batch size, then batch_size -> chunk size."""
    from clsurvey_amd.data import TensorTaskDataset
    from clsurvey_amd.methods import gem_main
    ref = _g35()["triples"]
    dsets = {"train": TensorTaskDataset(torch.zeros(I.TRIPLE_TRAIN, 1, 1, 1), torch.zeros(I.TRIPLE_TRAIN), []),
             "val": TensorTaskDataset(torch.zeros(7, 1, 1, 1), torch.zeros(7), [])}
    prev = tmp_path / "prev.pth"
    prev.write_bytes(b"0")
    seen = {}

    class Stub:
        batch_size, n_tasks, n_outputs = 10 ** 6, I.TRIPLE_TASKS, I.TRIPLE_NC * I.TRIPLE_TASKS

        def __init__(self, *a, **k):
            pass

        def init_setup(self, args):
            pass

    def recorder(model, args, dset_sizes, resume=""):
        seen["r"] = [args.dset_loaders["train"].batch_size, args.batch_size, args.n_exemplars_to_append_per_batch]
        return None, 0.0
    monkeypatch.setattr(gem_main, "train_model", recorder)
    monkeypatch.setattr(gem_main.R, "RehearsalNet", Stub)
    monkeypatch.setattr(gem_main.R, "replace_head", lambda m, n: m)
    monkeypatch.setattr(gem_main.torch, "load", lambda *a, **k: Stub())
    for method in ("baseline_rehearsal_partial_mem", "baseline_rehearsal_full_mem"):
        for task in (1, 2, 3):
            kw = dict(weight_decay=0.0, task_name=str(task), task_count=task, prev_model_path=str(prev), save_path=str(tmp_path),
                      n_outputs=I.TRIPLE_NC * I.TRIPLE_TASKS, method=method, n_memories=I.TRIPLE_MEM, n_epochs=1, cuda=True,
                      dataset_path=dsets, n_tasks=I.TRIPLE_TASKS, batch_size=I.TRIPLE_BATCH, lr=0.01, finetune=True,
                      is_scratch_model=task == 1)
            gem_main.main(kw, [I.TRIPLE_NC] * I.TRIPLE_TASKS, device="cpu")
            assert seen["r"] == ref["%s/task%d" % (method, task)], (method, task)


def _cpu_wrapper(spec):
    """RehearsalNet's host state (counters, store) without an engine."""
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.full_mem_mode, w.n_tasks = spec["full"], I.N_TASKS
    w.n_total_memories = spec["n_memories"] * I.N_TASKS
    w.n_memories = w.n_total_memories if spec["full"] else spec["n_memories"]
    w.observed_tasks, w.old_task, w.mem_cnt, w.filled = [], -1, 0, [0] * I.N_TASKS
    w.store_x = torch.zeros((w.n_total_memories, 1))
    w.store_y = torch.zeros(w.n_total_memories, dtype=torch.int64)
    return w


@pytest.mark.parametrize("tag", sorted(I.RUNS))
def test_sample_plan_and_memory_match_g35(tag):
    """The host plan reproduces the reference's per-task counts, slots and chunk orders at every step (same random /
    torch seeds); ring counter, n_memories, full-memory truncation and the stored labels match."""
    from clsurvey_amd.methods.rehearsal import sample_plan
    spec, steps = I.RUNS[tag], _g35()["runs"][tag]
    npz = np.load(os.path.join(HERE, "golden", "G35_rehearsal_baselines.npz"))
    data = I.batches(spec["seed"] + 4)
    w = _cpu_wrapper(spec)
    torch.manual_seed(spec["seed"] + 2)
    random.seed(spec["seed"] + 3)
    for k, rec in enumerate(steps):
        t = rec["t"]
        n_append, chunk = spec["append"][t]
        if t != w.old_task:
            w.switch_task(t)
        y = torch.from_numpy(data[k][1])
        row0, eff = w.ring_update(t, len(y))
        w.store_y[row0:row0 + eff] = y[:eff]
        counts, plan = sample_plan(t, n_append, w.observed_tasks, w.n_memories, chunk, w.filled)
        assert [(p, s, c) for p, s, c in plan] == [(p["task"], p["slots"], p["chunks"]) for p in rec["plan"]], (tag, k)
        assert [counts[p["task"]] for p in rec["plan"]] == [len(p["slots"]) for p in rec["plan"]]
        assert (w.mem_cnt, w.n_memories) == (rec["mem_cnt"], rec["n_memories"]), (tag, k)
        ref_labels = npz["%s_s%d_mem_labels" % (tag, k)]
        for task in w.observed_tasks:
            f, base = w.filled[task], task * w.n_memories
            assert (w.store_y[base:base + f].numpy() == ref_labels[task, :f]).all(), (tag, k, task)


def test_plan_errors_where_the_reference_would_hang_or_load_none():
    from clsurvey_amd.methods.rehearsal import sample_plan
    with pytest.raises(ValueError, match="never end"):
        sample_plan(1, 6, [0, 1], 5, 3)
    random.seed(0)
    with pytest.raises(ValueError, match="never filled"):
        sample_plan(1, 5, [0, 1], 5, 3, filled=[2, 0])


def test_new_abi_entries_reject_bad_arguments():
    from clsurvey_amd import _lib
    L = _lib.lib()
    assert L.clhip_rehearsal_assemble(None, None, -1, 16, None, None, 0, 0, 0, None, 0, None, None, None) == -1
    assert L.clhip_rehearsal_assemble(None, None, 2, 16, None, None, 0, 0, 0, None, 0, None, None, None) == -1
    assert L.clhip_rehearsal_assemble(None, None, 0, 0, None, None, 0, 0, 0, None, 0, None, None, None) == -1
    assert L.clhip_loss_segments(None, None, None, 0, 4, 8, None, 1, 1.0, None, None, None, None) == -1
    assert L.clhip_net_loss_step_loss_segments(None, None, None, None, None, None, 0, 4, None, 1, 1.0, None, None, None, None, None) == -1
