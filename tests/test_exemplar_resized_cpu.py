"""Resized replay of stored exemplars, the parts that need no GPU: the two new entry points and their argument errors, the
exemplar draws of a wrapper with a RandomResizedCropFlip spec (a function of the seed, windows inside each frame's own extent,
nothing taken from the global generators), the extents through the ring and a task switch, and the opt-in switch of
gem_main.main and of the driver."""
import ctypes as C
import os
import random

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY, ENTRY_U8 = "clhip_rehearsal_assemble_resized_crop_flip", "clhip_rehearsal_assemble_resized_crop_flip_u8"
EINVAL = -1


def test_symbols_are_exported_declared_and_in_the_signature_table():
    from clsurvey_amd import _lib
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        header = f.read()
    for entry in (ENTRY, ENTRY_U8):
        assert entry in _lib.SIGNATURES and hasattr(_lib.lib(), entry) and "int %s(" % entry in header
    assert _lib.SIGNATURES[ENTRY] == _lib.SIGNATURES["clhip_rehearsal_assemble_crop_flip"]
    assert _lib.SIGNATURES[ENTRY_U8] == _lib.SIGNATURES["clhip_rehearsal_assemble_crop_flip_u8"]
    assert len(_lib.SIGNATURES[ENTRY_U8][1]) == len(_lib.SIGNATURES[ENTRY][1]) + 1                # lut


def _enotsup():
    """What the resizing gather returns for a frame whose plan does not fit the LDS (1000 -> 125, include/clhip.h): the
    library's CLHIP_ENOTSUP, returned before any launch."""
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)
    rc = _lib.lib().clhip_gather_tasks_resized_crop_flip(one, 1, 1, 1000, 1000, 125, 125, one, one, 1, one, one, None)
    assert rc not in (0, EINVAL)
    return rc


@pytest.mark.parametrize("entry", [ENTRY, ENTRY_U8])
def test_argument_errors_do_not_need_a_device(entry):
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = getattr(_lib.lib(), entry)
    u8 = entry == ENTRY_U8

    def call(x=one, y=one, B=4, geo=(3, 20, 20, 16, 16), lut=one, src=one, src_rows=9, src_idx=one, store=one, store_y=one,
             store_rows=12, row0=2, ring=3, gather=one, params=one, E=2, x_mix=one, y_mix=one):
        table = (lut,) if u8 else ()
        return f(x, y, B, *geo, *table, src, src_rows, src_idx, store, store_y, store_rows, row0, ring, gather, params, E, x_mix,
                 y_mix, None)
    # what clhip_rehearsal_assemble refuses
    assert call(B=-1) == EINVAL and call(E=-1) == EINVAL and call(ring=-1) == EINVAL and call(store_rows=-1) == EINVAL
    assert call(ring=5) == EINVAL                                 # ring rows are a prefix of the batch
    assert call(x=None) == EINVAL and call(y=None) == EINVAL and call(y_mix=None) == EINVAL
    assert call(store=None) == EINVAL and call(store_y=None) == EINVAL and call(gather=None) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=10) == EINVAL
    assert call(B=70000, ring=0) == EINVAL
    # the geometry rule of clhip_gather_tasks_resized_crop_flip, and the frame-mode arguments
    for geo in ((0, 20, 20, 16, 16), (3, 0, 20, 16, 16), (3, 20, 0, 16, 16), (3, 20, 20, 0, 16), (3, 20, 20, 16, 0), (3, 20, 20, -1, 16)):
        assert call(geo=geo) == EINVAL, geo
    assert call(params=None) == EINVAL and call(src=None) == EINVAL and call(src_idx=None) == EINVAL and call(src_rows=-1) == EINVAL
    assert call(x_mix=None) == EINVAL                             # x_mix may be missing only without exemplars
    assert call(B=0, ring=0, E=0) == 0                            # nothing to do
    assert call(B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0    # the ring-only form with an empty ring
    # an output larger than the frame is an enlargement, not an error (the crop entry refuses it)
    assert call(geo=(3, 5, 7, 8, 8), B=0, ring=0, E=0) == 0
    # the plan: needed exactly when exemplars are resampled
    big = (1, 1000, 1000, 125, 125)
    assert call(geo=big) == _enotsup() and call(geo=big, B=0, ring=0, E=1) == _enotsup()
    assert call(geo=big, B=0, ring=0, E=0) == 0
    assert call(geo=big, B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0
    if u8:                                                        # the table: needed exactly when exemplars are decoded
        assert call(lut=None) == EINVAL and call(lut=None, B=0, ring=0, E=1) == EINVAL
        assert call(lut=None, B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0 and call(lut=None, B=0, ring=0, E=0) == 0


# ---------------------------------------------------------------------------------------------- the host side of a wrapper
FRAME, CROP = (1, 9, 11), (5, 6)


def _spec(**kw):
    from clsurvey_amd.data import RandomResizedCropFlip
    return RandomResizedCropFlip(CROP, **kw)


def _host_wrapper(spec=None, full=False, n_tasks=3, n_mem=6):
    """A RehearsalNet without net and engine: the host side of the store (as test_exemplar_augment_cpu._host_wrapper)."""
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.device = torch.device("cpu")
    w.in_shape = (FRAME[0],) + CROP
    w._init_frames(_spec() if spec is None else spec, FRAME)
    w.full_mem_mode, w.n_tasks, w.n_total_memories = full, n_tasks, n_mem * n_tasks
    w.n_memories = w.n_total_memories if full else n_mem
    w.observed_tasks, w.old_task, w.mem_cnt, w.filled = [], -1, 0, [0] * n_tasks
    w.n_append, w.chunk_size = 0, 4
    w._load_rows({})
    return w


def _source(ext, idx):
    from clsurvey_amd.methods.exemplar import BatchSource
    idx = torch.tensor(idx, dtype=torch.int64)
    return BatchSource(torch.zeros((10 if ext is None else len(ext),) + FRAME), idx, idx, ext)


def test_init_frames_keeps_the_spec_without_its_extents():
    from clsurvey_amd.data import RandomResizedCropFlip
    spec = _spec(scale=(0.3, 0.9), ratio=(0.5, 1.5), p=0.25, extents=torch.tensor([[9, 11]] * 4))
    w = _host_wrapper(spec)
    t = w.exemplar_transform
    assert isinstance(t, RandomResizedCropFlip) and t is not spec and t.extents is None
    assert (t.size, t.scale, t.ratio, t.p) == (CROP, (0.3, 0.9), (0.5, 1.5), 0.25)
    assert w.frame_shape == FRAME and w.store_shape == FRAME and w.geometry == FRAME + CROP and w.params_width == 5
    assert tuple(w.store_x.shape) == (18,) + FRAME and w.store_ext.tolist() == [[9, 11]] * 18


def test_init_frames_rejects_any_other_transform_and_smaller_frames():
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.in_shape = (FRAME[0],) + CROP
    for other in (object(), "RandomResizedCropFlip", (5, 6), lambda x: x):
        with pytest.raises(TypeError, match="exemplar_transform is a RandomCropFlip and comes with the frame shape"):
            w._init_frames(other, FRAME)
    with pytest.raises(TypeError):
        w._init_frames(_spec(), None)
    with pytest.raises(ValueError):
        w._init_frames(_spec(), (1, 4, 11))                       # a frame smaller than the net's input
    with pytest.raises(ValueError):
        w._init_frames(_spec(), (2, 9, 11))                       # another channel count
    assert w.exemplar_transform is None and w.frame_shape is None


def _filled_wrapper():
    w = _host_wrapper()
    w.observed_tasks, w.old_task, w.filled = [0, 1, 2], 2, [6, 6, 0]
    w.n_append, w.chunk_size = 7, 3
    g = torch.Generator().manual_seed(1)
    w.store_ext[:12] = torch.stack([torch.randint(5, 10, (12,), generator=g), torch.randint(6, 12, (12,), generator=g)], 1)
    return w


def _planned(w, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    seeds = []
    _, plan = w.plan(2, seeds)
    gather = [w._row(past, s) for past, _, chs in plan for ch in chs for s in ch]
    return gather, w.exemplar_params(gather, seeds), seeds, torch.get_rng_state(), random.getstate()


def test_exemplar_draws_are_resized_windows_inside_their_own_extents():
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    w = _filled_wrapper()
    seen = set()
    for seed in range(30):
        gather, params, seeds, _, _ = _planned(w, seed)
        again = _planned(w, seed)
        assert len(gather) == 7 and again[0] == gather and torch.equal(again[1], params)
        assert params.dtype == torch.int32 and tuple(params.shape) == (7, 5) and params.is_contiguous()
        ext = w.store_ext[torch.tensor(gather)]
        assert torch.equal(params, w.draw_exemplar_params(ext, seeds[-1]))
        want = draw_resized_crop_flip(7, RandomResizedCropFlip(CROP, extents=ext), FRAME[1:], torch.Generator().manual_seed(seeds[-1]))
        assert torch.equal(params, want)
        p = params.long()
        assert bool((p[:, :2] >= 0).all()) and bool((p[:, 2:4] >= 1).all())
        assert bool((p[:, 0] + p[:, 2] <= ext[:, 0]).all()) and bool((p[:, 1] + p[:, 3] <= ext[:, 1]).all())
        assert bool(((p[:, 4] == 0) | (p[:, 4] == 1)).all())
        seen.update(map(tuple, p.tolist()))
    assert len(seen) > 40 and {r[4] for r in seen} == {0, 1} and len({r[2:4] for r in seen}) > 5


def test_the_draws_leave_the_global_generators_alone():
    """The plan consumes the generators as the crop spec's does; the draws themselves take nothing."""
    from clsurvey_amd.data import RandomCropFlip
    a, b = _filled_wrapper(), _filled_wrapper()
    b.exemplar_transform = RandomCropFlip(CROP, 0.5)
    for seed in (0, 5, 9):
        ga, pa, _, ta, ra = _planned(a, seed)
        gb, pb, _, tb, rb = _planned(b, seed)
        assert ga == gb and tuple(pa.shape) == (7, 5) and tuple(pb.shape) == (7, 3)
        assert torch.equal(ta, tb) and ra == rb
    torch.manual_seed(3)
    random.seed(3)
    before, before_py = torch.get_rng_state(), random.getstate()
    out = a.draw_exemplar_params(a.store_ext[:12], 77)
    assert tuple(out.shape) == (12, 5) and torch.equal(before, torch.get_rng_state()) and before_py == random.getstate()
    assert tuple(a.exemplar_params([], []).shape) == (0, 5)


def test_ring_update_and_switch_task_carry_the_extents():
    """Partial memory: the ring and its wrap; full memory: the compaction at a task switch.  As with a crop spec."""
    w = _host_wrapper()
    ext = torch.tensor([[5 + k % 5, 6 + k % 6] for k in range(10)])
    w.switch_task(0)
    assert w.ring_update(0, 4, _source(ext, [7, 2, 9, 0])) == (0, 4)
    assert w.ring_update(0, 4, _source(ext, [1, 3, 5, 8])) == (4, 2)                # wraps
    assert w.store_ext[:6].tolist() == ext[[7, 2, 9, 0, 1, 3]].tolist() and w.store_ext[6:].tolist() == [[9, 11]] * 12
    w.switch_task(1)
    assert w.ring_update(1, 4, _source(None, [0, 1, 2, 3])) == (6, 4) and w.store_ext[6:10].tolist() == [[9, 11]] * 4
    f = _host_wrapper(full=True)
    f.switch_task(0)
    row0, eff = f.ring_update(0, 5, _source(ext, [3, 1, 4, 9, 5]))
    assert (row0, eff) == (0, 5)
    f.switch_task(1)                                                                # 18 rows -> 9 + 9: task 0 keeps its 5
    assert f.n_memories == 9 and f.filled == [5, 0, 0] and f.store_ext[:5].tolist() == ext[[3, 1, 4, 9, 5]].tolist()
    assert f.ring_update(1, 3, _source(ext, [0, 6, 2])) == (9, 3) and f.store_ext[9:12].tolist() == ext[[0, 6, 2]].tolist()
    assert f._rows_state()["_rows_ext"].tolist() == f.store_ext.tolist()


# ---------------------------------------------------------------------------------------------- the switch
def _args(root, method, train, val, **kw):
    prev = os.path.join(root, "prev.pth.tar")
    torch.save({}, prev)
    return dict(task_name="2", task_count=2, prev_model_path=prev, n_outputs=8, method=method, n_memories=4, n_tasks=2,
                dataset_path={"train": train, "val": val, "test": val}, postprocess=False, is_scratch_model=False, **kw)


@pytest.mark.parametrize("method", ["gem", "baseline_rehearsal_full_mem", "baseline_rehearsal_partial_mem"])
def test_without_the_switch_the_entry_still_refuses_and_names_it(tmp_path, method):
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip, TensorTaskDataset
    from clsurvey_amd.methods import gem_main
    x, y = torch.zeros((4, 3, 16, 16)), torch.tensor([0, 1, 2, 3])
    plain = TensorTaskDataset(x[:, :, :8, :8], y, list("abcd"))
    resized = TensorTaskDataset(x, y, list("abcd"), transform=RandomResizedCropFlip((8, 8)))
    for extra in ({}, {"exemplar_resized": False}):
        with pytest.raises(NotImplementedError, match="RandomCropFlip only.*RandomResizedCropFlip.*exemplar_resized=True.*--resized_exemplars"):
            gem_main.main(_args(str(tmp_path), method, resized, plain, **extra), [4, 4], device="cpu")
    # the switch belongs to a resized split: on any other one it is an error raised before any loader or device is touched
    crop = TensorTaskDataset(x, y, list("abcd"), transform=RandomCropFlip((8, 8)))
    for train in (crop, plain):
        with pytest.raises(ValueError, match="exemplar_resized=True"):
            gem_main.main(_args(str(tmp_path), method, train, plain, exemplar_resized=True), [4, 4], device="cpu")


def test_the_switch_does_not_open_a_byte_store_for_float_frames(tmp_path):
    """exemplar_dtype='uint8' keeps asking for a ByteTaskDataset, with the switch too; byte frames keep asking for a byte store."""
    from clsurvey_amd.data import ByteTaskDataset, RandomResizedCropFlip, TensorTaskDataset
    from clsurvey_amd.methods import gem_main
    xb = torch.randint(0, 256, (4, 3, 16, 16), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    y = torch.tensor([0, 1, 2, 3])
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    plain = TensorTaskDataset(torch.zeros((4, 3, 8, 8)), y, list("abcd"))
    floats = TensorTaskDataset(torch.zeros((4, 3, 16, 16)), y, list("abcd"), transform=RandomResizedCropFlip((8, 8)))
    with pytest.raises(ValueError, match="exemplar_dtype='uint8'.*ByteTaskDataset carrying a RandomCropFlip"):
        gem_main.main(_args(str(tmp_path), "gem", floats, plain, exemplar_resized=True, exemplar_dtype="uint8"), [4, 4], device="cpu")
    byte = ByteTaskDataset(xb, y, list("abcd"), *norm, transform=RandomResizedCropFlip((8, 8)))
    with pytest.raises(NotImplementedError, match="byte frames.*exemplar_dtype='uint8'"):
        gem_main.main(_args(str(tmp_path), "gem", byte, plain, exemplar_resized=True), [4, 4], device="cpu")


def test_resized_exemplars_without_rnd_resized_is_a_system_exit(tmp_path):
    from clsurvey_amd.framework import driver
    argv = ["small_VGG9_cl_128_128", "--results_root", str(tmp_path), "--synthetic", "2,4,16,8,8,32", "--method_name",
            "finetuning_rehearsal_partial_mem", "--mem_per_task", "4", "--resized_exemplars"]
    for extra in ([], ["--rnd_margin", "4"]):
        with pytest.raises(SystemExit, match="--resized_exemplars belongs with --rnd_resized"):
            driver.main(argv + extra)
    # a byte store on resized tasks needs both switches
    with pytest.raises(SystemExit, match="--u8_exemplars belongs with"):
        driver.main([a for a in argv if a != "--resized_exemplars"] + ["--rnd_resized", "4", "--u8_frames", "--u8_exemplars"])
    assert not os.path.exists(os.path.join(str(tmp_path), "data"))                   # raised before anything is generated
