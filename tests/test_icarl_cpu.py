"""iCaRL without a GPU, against fixture G37 (tests/golden/make_g37.py): the method-table row, the host draws and segment
scales of update_representation, the mean weights, main_rehearsal's batch split through the iCaRL trainer, the poststep
paths over a stand-in trainer, and argument errors of the new ABI entries."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g37_common as I  # noqa: E402


def _g37():
    with open(os.path.join(HERE, "golden", "G37_icarl.json")) as f:
        return json.load(f)


def test_method_row_matches_g37():
    from clsurvey_amd.methods import method as M
    row = _g37()["method"]
    m = M.parse("ICARL")
    assert type(m).__name__ == row["class"] and M.ICARL is type(m)
    assert (m.name, m.eval_name, m.extra_hyperparams_count) == (row["name"], row["eval_name"], row["extra_hyperparams_count"])
    assert m.category.name == row["category"]
    assert list(m.hyperparams.items()) == [tuple(kv) for kv in row["hyperparams"]]
    assert list(m.static_hyperparams.items()) == [tuple(kv) for kv in row["static_hyperparams"]]
    for flag in ("start_scratch", "no_framework", "grid_chkpt", "wrap_first_task_model"):
        assert bool(getattr(m, flag, False)) == bool(row["flags"].get(flag, False)), flag
    for hook in row["hooks"]:
        assert callable(getattr(m, hook, None)), hook
    assert m.spec["output"] == "icarl_nme" and m.spec["evaluate"] == "as_is" and m.spec["phase1"] is None


def test_gem_main_still_refuses_icarl():
    from clsurvey_amd.methods import gem_main
    with pytest.raises(NotImplementedError, match="icarl_main"):
        gem_main.main(dict(method="icarl", task_count=1, prev_model_path="x", n_tasks=1), [2])
    from clsurvey_amd.methods import icarl_main
    with pytest.raises(NotImplementedError):
        icarl_main.main(dict(method="gem", task_count=1, prev_model_path="x", n_tasks=1), [2])


def test_mean_weights():
    from clsurvey_amd.methods.icarl import mean_weights
    npz = np.load(os.path.join(HERE, "golden", "G37_icarl.npz"))
    for t in range(I.N_TASKS):
        for c, n in enumerate(I.CLASS_SIZES[t]):
            w = mean_weights(n, I.HERD_BATCH)
            assert np.array_equal(w, npz["m%d_c%d_w" % (t, c)])
            assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
    w = mean_weights(5, 2)                    # batches 2, 2, 1: the last row weighs twice as much
    assert np.allclose(w, [1 / 6] * 4 + [1 / 3])


def test_segment_scales_mirror_the_accumulation_as_written():
    """T_1 = reg A_1 / c_1, T_2 = reg (T_1 + A_2) / (c_1 + c_2), ...; loss += sum_j T_j."""
    from clsurvey_amd.methods.icarl import segment_scales
    rng = np.random.RandomState(0)
    for counts, reg in (([2, 2], 1.5), ([1], 10.0), ([2, 1, 3], 0.7)):
        losses = [rng.rand(c) for c in counts]
        total, count, add = 0.0, 0, 0.0
        for ch in losses:                          # icarl.py:565-592
            for v in ch:
                total += v
                count += 1
            total = reg * (total / count)
            add += total
        scales = segment_scales(counts, reg)
        assert abs(sum(s * ch.sum() for s, ch in zip(scales, losses)) - add) <= 1e-12 * abs(add)
    assert np.allclose(segment_scales([2, 1], 10.0), [5 + 50 / 3, 10 / 3])


def test_segment_scales_match_g37_losses():
    """G37 records, per task-3 step, the CE of the current batch, every chunk's distillation loss as computed, before the
    negative-chunk rule (two past tasks, one or two chunks each) and the loss the reference stepped on: CE + sum of scale(task) * chunk loss reproduces it within two
    fp32 ulps of the recorded loss (2 * 2^-23 * 1.4 < 2.5e-7; the distillation part is ~1e-4 to 4e-4 here), which the
    accumulation with a reset per task misses by more than ten times that."""
    from clsurvey_amd.methods.icarl import segment_scales
    for rec in _g37()["steps"]:
        counts = [len(p["chunks"]) for p in rec["plan"]]
        assert len(counts) == 2 and sum(counts) == len(rec["chunk_losses"])
        scales = segment_scales(counts, I.REG)
        per_chunk = [s for s, c in zip(scales, counts) for _ in range(c)]
        total = rec["ce"] + sum(s * (v if v >= 0 else 0.0) for s, v in zip(per_chunk, rec["chunk_losses"]))     # :584-587
        assert abs(total - rec["loss"]) <= 2.5e-7, (total, rec["loss"])
        intended = rec["ce"] + I.REG * sum(sum(rec["chunk_losses"][sum(counts[:j]):sum(counts[:j + 1])]) / counts[j] for j in range(2))
        assert abs(intended - rec["loss"]) > 10 * 2.5e-7          # the paper's reset-per-task form is NOT what was recorded


def test_host_draws_match_g37():
    """Same seeds of random / numpy / torch as the generator: the chunks (class, exemplar index) of every recorded step."""
    from clsurvey_amd.methods.icarl import exemplar_draws
    ref = _g37()
    assert [m["exemplar_count"] for m in ref["manage"]] == [6, 3, 2]
    class_len = [3] * 8                           # after manage_memory(1)
    cum = [4, 8, 12]
    # the unrecorded steps of task 2 consume draws from their own seeds; the recorded ones start from seed_draws(2)
    I.seed_draws(2)
    for rec in ref["steps"]:
        counts, plan = exemplar_draws(2, I.N_APPEND, class_len, 3, I.NC_PER_TASK, cum, I.TOTAL_BATCH)
        assert sum(counts) == I.N_APPEND
        assert [(p, [[list(r) for r in ch] for ch in chunks]) for p, chunks in plan] == [(p["task"], p["chunks"]) for p in rec["plan"]]
        assert any(len(chunks) > 1 for _, chunks in plan)


def test_draws_capped_branch_and_endless_redraw():
    from clsurvey_amd.methods.icarl import exemplar_draws
    import random
    state = random.getstate()
    counts, plan = exemplar_draws(1, 40, [2, 2, 2, 2], 2, [4, 4], [4, 8], 8)     # floor(40 / 4) > 2: capped, no random draw
    assert counts == [2, 2, 2, 2] and random.getstate() == state
    assert sorted(r for ch in plan[0][1] for r in ch) == [(c, e) for c in range(4) for e in range(2)]
    with pytest.raises(ValueError, match="never end"):
        exemplar_draws(1, 11, [2, 2, 2, 2], 2, [4, 4], [4, 8], 8)                # 2 each + 3 leftovers, every class full
    assert exemplar_draws(1, 4, [], 0, [4, 4], [4, 8], 8) == ([], [])


def test_batch_split_through_icarl_main(monkeypatch, tmp_path):
    """main_rehearsal.py:181-202: loaders at the ORIGINAL batch size, then the full-memory ratio for 'icarl'."""
    from clsurvey_amd.data import TensorTaskDataset
    from clsurvey_amd.methods import icarl_main
    n_train, batch, mem, tasks, nc = 300, 64, 40, 4, 3
    dsets = {"train": TensorTaskDataset(torch.zeros(n_train, 1, 1, 1), torch.zeros(n_train), []),
             "val": TensorTaskDataset(torch.zeros(7, 1, 1, 1), torch.zeros(7), [])}
    prev = tmp_path / "SI_prev.pth"
    prev.write_bytes(b"0")
    seen = {}

    class Stub:
        batch_size, n_tasks, n_outputs = 10 ** 6, tasks, nc * tasks

        def __init__(self, *a, **k):
            if len(a) > 8:
                seen["rows"] = a[8]

        def init_setup(self, args):
            pass

        def manage_memory(self, t, args):
            seen["r"] = [args.dset_loaders["train"].batch_size, args.batch_size, args.n_exemplars_to_append_per_batch,
                         args.total_batch_size]

    def recorder(model, args, dset_sizes, resume=""):
        seen["r"] = [args.dset_loaders["train"].batch_size, args.batch_size, args.n_exemplars_to_append_per_batch, args.total_batch_size]
        return None, 0.0
    monkeypatch.setattr(icarl_main.gem_main, "train_model", recorder)
    monkeypatch.setattr(icarl_main.I, "IcarlNet", Stub)
    monkeypatch.setattr(icarl_main.torch, "load", lambda *a, **k: Stub())
    monkeypatch.setattr(icarl_main.torch, "save", lambda *a, **k: None)
    n_append = int(np.ceil(batch * (mem * tasks) / (n_train + mem * tasks)))
    for task in (1, 2, 3):
        kw = dict(weight_decay=0.0, task_name=str(task), task_count=task, prev_model_path=str(prev), save_path=str(tmp_path / "o" / "m.pth"),
                  n_outputs=nc * tasks, method="icarl", n_memories=mem, n_epochs=1, cuda=True, dataset_path=dsets, n_tasks=tasks,
                  batch_size=batch, lr=0.01, finetune=task > 1, is_scratch_model=task == 1, postprocess=task == 1,
                  memory_strength=1.0)
        icarl_main.main(kw, [nc] * tasks, device="cpu")
        assert seen["r"] == [batch, batch - n_append, n_append, batch], task
    assert seen["rows"] == batch + n_append
    with pytest.raises(AssertionError, match="POSTPROCESSING"):
        icarl_main.main(dict(kw, task_count=1, postprocess=False), [nc] * tasks, device="cpu")


def test_poststep_paths(monkeypatch, tmp_path):
    """Task 1 wraps into manager.best_model_path from the shared SI model; task 2 writes best_model_postprocessed.pth.tar beside
    the trained model, from it; an existing file is not redone; best_model_path moves to the postprocessed file."""
    from clsurvey_amd.methods import method as M
    calls = []

    def stand_in(kw, nc, device="cuda"):
        calls.append(dict(kw))
        if kw["postprocess"]:
            os.makedirs(os.path.dirname(kw["save_path"]), exist_ok=True)
            open(kw["save_path"], "wb").close()
        return None, None
    monkeypatch.setattr(M._icarl, "main", stand_in)
    m = M.parse("ICARL")
    ds = types.SimpleNamespace(classes_per_task={"1": [0, 1], "2": [0, 1, 2]}, task_count=2)
    t1 = str(tmp_path / "task_1" / "TASK_TRAINING")
    t2 = str(tmp_path / "task_2" / "TASK_TRAINING")
    manager = types.SimpleNamespace(dataset=ds, best_model_path=os.path.join(t1, "best_model.pth.tar"), heuristic_exp_dir=t1,
                                    previous_task_model_path="/x/SI/best_model.pth.tar", current_task_dataset_path="d1")
    args = types.SimpleNamespace(task_counter=1, weight_decay=0.0, task_name="1", num_epochs=2, batch_size=8, device="cpu")
    m.poststep(args, manager)
    assert len(calls) == 1 and calls[0]["postprocess"] and calls[0]["is_scratch_model"] and calls[0]["method"] == "icarl"
    assert calls[0]["prev_model_path"] == "/x/SI/best_model.pth.tar" and calls[0]["save_path"] == os.path.join(t1, "best_model.pth.tar")
    assert calls[0]["memory_strength"] == 10 and calls[0]["n_memories"] == 1024 and calls[0]["n_outputs"] == 5
    assert calls[0]["lr"] == 0.0 and args.postprocess_time >= 0
    assert manager.best_model_path == os.path.join(t1, "best_model.pth.tar")
    manager.heuristic_exp_dir = t2
    manager.best_model_path = os.path.join(t2, "best_model.pth.tar")
    manager.previous_task_model_path = os.path.join(t1, "best_model.pth.tar")
    manager.current_task_dataset_path = "d2"
    args.task_counter, args.task_name, args.lr = 2, "2", 0.01
    m.poststep(args, manager)
    post = os.path.join(t2, "best_model_postprocessed.pth.tar")
    assert len(calls) == 2 and calls[1]["prev_model_path"] == os.path.join(t2, "best_model.pth.tar")
    assert calls[1]["save_path"] == post and calls[1]["postprocess"] and not calls[1]["is_scratch_model"] and calls[1]["lr"] == 0.01
    assert manager.best_model_path == post and m.postprocessed_model_name == os.path.basename(post)
    manager.best_model_path = os.path.join(t2, "best_model.pth.tar")
    m.poststep(args, manager)                         # the file exists: skipped
    assert len(calls) == 2 and manager.best_model_path == post
    # phase 1 / phase 2 reach the same trainer
    manager.gridsearch_exp_dir = str(tmp_path / "grid")
    m.grid_train(args, manager, 0.05)
    assert calls[2]["finetune"] and calls[2]["memory_strength"] == 0 and calls[2]["lr"] == 0.05 and not calls[2]["postprocess"]
    m.train(args, manager, {"lambda": 2.5})
    assert not calls[3]["finetune"] and calls[3]["memory_strength"] == 2.5 and calls[3]["save_path"] == t2


def test_new_abi_entries_reject_bad_arguments():
    import ctypes as C
    from clsurvey_amd import _lib
    L = _lib.lib()
    tab = (_lib.IcarlClass * 1)()
    assert L.clhip_icarl_herd(None, 4, 8, None, tab, 1, None, 1, None) == -1
    buf = C.create_string_buffer(64)                  # (never dereferenced: every call below fails its checks first)
    p = C.addressof(buf)
    tab[0].row_begin, tab[0].row_end, tab[0].k, tab[0].out_off = 0, 5, 1, 0
    assert L.clhip_icarl_herd(p, 4, 8, p, tab, 1, p, 1, None) == -1            # rows outside feats
    tab[0].row_end, tab[0].k = 4, 5
    assert L.clhip_icarl_herd(p, 4, 8, p, tab, 1, p, 5, None) == -1            # more picks than rows
    tab[0].k = 2
    assert L.clhip_icarl_herd(p, 4, 8, p, tab, 1, p, 1, None) == -1            # ranking too short
    assert L.clhip_icarl_herd(p, 4, 5000, p, tab, 1, p, 2, None) == -1         # F over the LDS budget
    assert L.clhip_loss_segments(None, None, None, 0, 4, 8, None, 1, 2.0, None, None, None, None) == -1
    assert L.clhip_loss_segments(p, p, None, 0, 2000, 8, p, 1, 2.0, p, p, None, None) == -1
    assert L.clhip_net_loss_step_loss_segments(None, None, None, None, None, None, 0, 4, None, 1, 2.0, None, None, None, None, None) == -1
    assert L.clhip_icarl_nme(None, None, 4, 8, 4, 0, 12, None, None) == -1
    assert L.clhip_icarl_nme(None, None, 4, 8, 4, 10, 12, p, None) == -1       # slice outside the head
