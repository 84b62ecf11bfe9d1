"""Exemplars stored as frames and re-augmented at every replay, the parts that need no GPU: the new entry point and its
argument errors, the host bookkeeping of the stored frames' extents through a ring wrap and an R-FM compaction, and the
exemplar draws of a rehearsal step (a function of the seed, inside each frame's own extent, nothing taken from the global
generator)."""
import os
import random

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_symbol_is_exported_and_declared():
    from clsurvey_amd import _lib
    assert "clhip_rehearsal_assemble_crop_flip" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "clhip_rehearsal_assemble_crop_flip")
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        assert "int clhip_rehearsal_assemble_crop_flip(" in f.read()


def test_argument_errors_do_not_need_a_device():
    import ctypes as C
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = _lib.lib().clhip_rehearsal_assemble_crop_flip

    def call(x=one, y=one, B=4, geo=(3, 20, 20, 16, 16), src=one, src_rows=9, src_idx=one, store=one, store_y=one, store_rows=12,
             row0=2, ring=3, gather=one, params=one, E=2, x_mix=one, y_mix=one):
        return f(x, y, B, *geo, src, src_rows, src_idx, store, store_y, store_rows, row0, ring, gather, params, E, x_mix, y_mix, None)
    # what clhip_rehearsal_assemble refuses
    assert call(B=-1) == -1 and call(E=-1) == -1 and call(ring=-1) == -1 and call(store_rows=-1) == -1
    assert call(ring=5) == -1                                     # ring rows are a prefix of the batch
    assert call(x=None) == -1 and call(y=None) == -1 and call(y_mix=None) == -1
    assert call(store=None) == -1 and call(store_y=None) == -1 and call(gather=None) == -1
    assert call(row0=-1) == -1 and call(row0=10) == -1
    assert call(B=70000, ring=0) == -1
    # what clhip_gather_tasks_crop_flip refuses of the geometry, and the new arguments
    for geo in ((0, 20, 20, 16, 16), (3, 20, 20, 21, 16), (3, 20, 20, 16, 21), (3, 20, 20, 0, 16), (3, 20, 20, 16, 0)):
        assert call(geo=geo) == -1, geo
    assert call(params=None) == -1 and call(src=None) == -1 and call(src_idx=None) == -1 and call(src_rows=-1) == -1
    assert call(x_mix=None) == -1                                 # x_mix may be missing only without exemplars
    assert call(B=0, ring=0, E=0) == 0                            # nothing to do
    assert call(B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0    # the ring-only form with an empty ring


# ---------------------------------------------------------------------------------------------- store_ext
def _host_wrapper(full, n_tasks=3, n_mem=6, frame=(1, 9, 11), crop=(5, 6), p=0.5):
    """A RehearsalNet without net and engine: the host side of the store (as tests/test_gpu_rehearsal.py builds one)."""
    from clsurvey_amd.data import RandomCropFlip
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.device = torch.device("cpu")
    w.in_shape = (frame[0],) + crop
    w._init_frames(RandomCropFlip(crop, p), frame)
    w.full_mem_mode, w.n_tasks, w.n_total_memories = full, n_tasks, n_mem * n_tasks
    w.n_memories = w.n_total_memories if full else n_mem
    w.observed_tasks, w.old_task, w.mem_cnt, w.filled = [], -1, 0, [0] * n_tasks
    w.n_append, w.chunk_size = 0, 4
    w._load_rows({})
    return w


def _source(ext, idx):
    from clsurvey_amd.methods.exemplar import BatchSource
    idx = torch.tensor(idx, dtype=torch.int64)
    return BatchSource(torch.zeros((10 if ext is None else len(ext), 1, 9, 11)), idx, idx, ext)


def _task_extents(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(5, 10, (n,), generator=g), torch.randint(6, 12, (n,), generator=g)], 1)


def test_store_ext_follows_the_ring_and_its_wrap():
    """Partial memory, 6 slots per task: batches of 4 wrap the ring in the second step; the table equals a list restatement."""
    w = _host_wrapper(False)
    assert tuple(w.store_x.shape) == (18, 1, 9, 11) and tuple(w.store_ext.shape) == (18, 2) and w.store_ext.dtype == torch.int64
    assert w.store_ext.tolist() == [[9, 11]] * 18 and not w.store_ext.is_cuda
    want = [[9, 11] for _ in range(18)]
    for t in range(2):
        ext = _task_extents(10, 20 + t)
        w.switch_task(t)
        cnt = 0
        for idx in ([7, 2, 9, 0], [1, 3, 5, 8], [4, 6, 2, 7], [9, 9, 0, 1]):
            row0, eff = w.ring_update(t, 4, _source(ext, idx))
            assert row0 == t * 6 + cnt and eff == min(4, 6 - cnt)
            for i in range(eff):
                want[row0 + i] = ext[idx[i]].tolist()
            cnt = 0 if cnt + eff == 6 else cnt + eff
        assert w.store_ext.tolist() == want
    assert w.filled == [6, 6, 0]
    # no extents: full frames
    w.switch_task(2)
    w.ring_update(2, 4, _source(None, [0, 1, 2, 3]))
    assert w.store_ext[12:16].tolist() == [[9, 11]] * 4


def test_store_ext_follows_the_full_memory_compaction():
    """Full memory, 18 rows: task 0 owns all of them, then 9 + 9, then 6 + 6 + 6; at every switch the kept rows of every task move
    with their extents (compact_blocks), restated on lists."""
    w = _host_wrapper(True)
    want = [[9, 11] for _ in range(18)]
    stride, filled = 18, [0, 0, 0]
    marks = torch.arange(18, dtype=torch.float32)
    for t in range(3):
        if t:
            new = 18 // (t + 1)
            filled = [min(f, new) for f in filled]
            for k in range(t):                                    # block k: rows [k * stride, +filled[k]) -> k * new
                want[k * new:k * new + filled[k]] = want[k * stride:k * stride + filled[k]]
            stride = new
        w.switch_task(t)
        assert w.n_memories == stride and w.filled == filled
        ext = _task_extents(12, 40 + t)
        for idx in ([3, 1, 4, 11, 5], [9, 2, 6, 8, 3], [7, 0, 10, 2, 6]):
            row0, eff = w.ring_update(t, 5, _source(ext, idx))
            for i in range(eff):
                want[row0 + i] = ext[idx[i]].tolist()
            w.store_x[row0:row0 + eff] = marks[row0:row0 + eff, None, None, None] + 100 * t      # (what the launch would copy)
            filled[t] = max(filled[t], row0 - t * stride + eff)
        assert w.filled == filled and w.store_ext.tolist() == want
    # the frames moved with their extents: task 0's first rows still carry task 0's marks
    assert w.store_x[:6, 0, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert w.store_x[6:12, 0, 0, 0].tolist() == [109.0, 110.0, 111.0, 112.0, 113.0, 114.0]      # rows 9 .. 14 of the 9-row layout
    # the pickled rows carry the extents of the rows in use
    state = w._rows_state()
    assert state["_rows_ext"].tolist() == want[:18] and tuple(state["_rows_x"].shape) == (18, 1, 9, 11)


def test_a_wrapper_refuses_the_other_kind_of_batch():
    import pytest
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = _host_wrapper(False)
    with pytest.raises(ValueError):
        w._check_source(None)
    with pytest.raises(ValueError):
        w._check_source(_source(None, [0])._replace(frames=torch.zeros((4, 1, 9, 12))))       # another frame shape
    plain = RehearsalNet.__new__(RehearsalNet)
    assert plain.exemplar_transform is None and plain.frame_shape is None                     # class-level defaults: old pickles
    plain.in_shape = (1, 5, 6)
    assert plain.store_shape == (1, 5, 6)
    plain._check_source(None)
    with pytest.raises(ValueError):
        plain._check_source(_source(None, [0]))


# ---------------------------------------------------------------------------------------------- the exemplar draws
def _planned(w, seed):
    """One step's plan at task 2 and its draws from RNG state `seed`: (gather rows, params, global RNG state after)."""
    random.seed(seed)
    torch.manual_seed(seed)
    seeds = []
    _, plan = w.plan(2, seeds)
    gather = [w._row(past, s) for past, _, chs in plan for ch in chs for s in ch]
    params = w.exemplar_params(gather, seeds) if w.exemplar_transform is not None else None
    return gather, params, seeds, torch.get_rng_state(), random.getstate()


def _filled_wrapper(frame_mode=True):
    w = _host_wrapper(False)
    w.observed_tasks, w.old_task, w.filled = [0, 1, 2], 2, [6, 6, 0]
    w.n_append, w.chunk_size = 7, 3
    g = torch.Generator().manual_seed(1)
    w.store_ext[:12] = torch.stack([torch.randint(5, 10, (12,), generator=g), torch.randint(6, 12, (12,), generator=g)], 1)
    w.store_ext[3] = torch.tensor([5, 6])                                                      # no freedom
    if not frame_mode:
        w.exemplar_transform = None
    return w


def test_exemplar_draws_are_a_function_of_the_seed_inside_their_own_extents():
    w = _filled_wrapper()
    seen = set()
    for seed in range(40):
        gather, params, seeds, _, _ = _planned(w, seed)
        again = _planned(w, seed)
        assert len(gather) == 7 and again[0] == gather and torch.equal(again[1], params)
        assert params.dtype == torch.int32 and tuple(params.shape) == (7, 3) and params.is_contiguous()
        assert len(seeds) == 2                                      # one base seed per exemplar loader; the last one seeds the draws
        assert torch.equal(params, w.draw_exemplar_params(w.store_ext[torch.tensor(gather)], seeds[-1]))
        ext = w.store_ext[torch.tensor(gather)]
        p = params.long()
        assert bool((p[:, 0] >= 0).all()) and bool((p[:, 0] <= ext[:, 0] - 5).all())
        assert bool((p[:, 1] >= 0).all()) and bool((p[:, 1] <= ext[:, 1] - 6).all())
        assert bool(((p[:, 2] == 0) | (p[:, 2] == 1)).all())
        for g, row in zip(gather, p.tolist()):
            if g == 3:
                assert row[:2] == [0, 0]
        seen.update(map(tuple, p.tolist()))
    assert len(seen) > 20 and {r[2] for r in seen} == {0, 1}
    assert not torch.equal(_planned(w, 1)[1], _planned(w, 2)[1])


def test_frame_mode_plan_consumes_the_generators_as_crop_mode_does():
    a, b = _filled_wrapper(True), _filled_wrapper(False)
    for seed in (0, 5, 9):
        ga, pa, _, ta, ra = _planned(a, seed)
        gb, pb, _, tb, rb = _planned(b, seed)
        assert ga == gb and pa is not None and pb is None
        assert torch.equal(ta, tb) and ra == rb


def test_an_empty_plan_draws_nothing():
    w = _filled_wrapper()
    w.n_append = 0
    seeds = []
    torch.manual_seed(3)
    before = torch.get_rng_state()
    assert w.plan(2, seeds) == ([], []) and seeds == []
    assert tuple(w.exemplar_params([], seeds).shape) == (0, 3) and torch.equal(before, torch.get_rng_state())
