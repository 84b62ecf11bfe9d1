"""iCaRL on augmented tasks, the parts that need no GPU: the four step-assembly entries and their argument errors, the host
bookkeeping of the stored frames' extents through two truncations, the herding view and the class-mean view (functions of
(view_seed, t), inside each frame's own extent, nothing taken from a global generator), the `seeds` argument of the exemplar
draws, and the argument rules of icarl_main.main that are decided before a device is needed."""
import os
import random
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ["clhip_icarl_assemble_crop_flip", "clhip_icarl_assemble_crop_flip_u8", "clhip_icarl_assemble_resized_crop_flip",
           "clhip_icarl_assemble_resized_crop_flip_u8"]


def test_symbols_are_exported_and_declared():
    from clsurvey_amd import _lib, ops
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        assert "int %s(" % name in header
        assert callable(getattr(ops, name[len("clhip_"):]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_do_not_need_a_device(entry):
    import ctypes as C
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    # (every call below is refused, or has B = E = 0: none reaches a launch, with or without a device)
    f = getattr(_lib.lib(), entry)
    u8, resized = entry.endswith("_u8"), "resized" in entry

    def call(x=one, y=one, B=4, geo=(3, 20, 20, 16, 16), lut=one, store=one, store_rows=12, gather=one, params=one, E=2, store_t=one,
             n_outputs=12, x_mix=one, y_mix=one, t_mix=one):
        table = (lut,) if u8 else ()
        return f(x, y, B, *geo, *table, store, store_rows, gather, params, E, store_t, n_outputs, x_mix, y_mix, t_mix, None)
    EINVAL, ENOTSUP = -1, -3
    assert call(B=-1) == EINVAL and call(E=-1) == EINVAL and call(store_rows=-1) == EINVAL              # negative counts
    for geo in ((0, 20, 20, 16, 16), (3, 0, 20, 16, 16), (3, 20, 0, 16, 16), (3, 20, 20, 0, 16), (3, 20, 20, 16, 0)):
        assert call(geo=geo) == EINVAL, geo
    assert call(n_outputs=0) == EINVAL and call(n_outputs=-4) == EINVAL
    for geo in ((3, 20, 20, 21, 16), (3, 20, 20, 16, 21)):        # a crop larger than the frame; a resized window may be enlarged
        assert call(geo=geo, B=0, E=0) == (0 if resized else EINVAL), geo
    # missing pointers for a non-zero count
    for name in ("x", "y", "x_mix", "y_mix"):
        assert call(**{name: None}) == EINVAL, name
        assert call(E=0, **{name: None}) == EINVAL, name
    for name in ("store", "gather", "params", "store_t", "t_mix"):
        assert call(**{name: None}) == EINVAL, name
        assert call(B=0, **{name: None}) == EINVAL, name
        assert call(B=0, E=0, **{name: None}) == 0, name         # ... and none of them is needed without exemplars
    assert call(B=0, x_mix=None) == EINVAL and call(B=0, y_mix=None) == EINVAL
    if u8:
        assert call(lut=None) == EINVAL and call(lut=None, B=0, E=0) == 0
    assert call(B=65530, E=6) == EINVAL and call(B=0, E=65536) == EINVAL and call(B=65536, E=0) == EINVAL
    if resized:                                                   # no plan fits the LDS: one output line of 8192 floats and its taps
        assert call(geo=(1, 4, 16384, 4, 8192)) == ENOTSUP
        assert call(geo=(1, 4, 16384, 4, 8192), E=0, B=0) == 0
    # the nothing-to-do forms
    assert call(B=0, E=0) == 0
    assert call(B=0, E=0, x=None, y=None, store=None, gather=None, params=None, store_t=None, x_mix=None, y_mix=None, t_mix=None) == 0


# ---------------------------------------------------------------------------------------------- store_ext
def _host_wrapper(n_tasks=3, n_mem=8, nc=2, frame=(1, 9, 11), crop=(5, 6), p=0.5, resized=False):
    """An IcarlNet without net and engine: the host side of the store (test_exemplar_augment_cpu.py's _host_wrapper)."""
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip
    from clsurvey_amd.methods.icarl import IcarlNet
    w = IcarlNet.__new__(IcarlNet)
    w.device = torch.device("cpu")
    w.in_shape = (frame[0],) + crop
    w._init_frames(RandomResizedCropFlip(crop, p=p) if resized else RandomCropFlip(crop, p), frame)
    w.n_outputs, w.n_tasks, w.n_total_memories = nc * n_tasks, n_tasks, n_mem * n_tasks
    w.nc_per_task = [nc] * n_tasks
    w.cum_nc_per_task = [nc * (i + 1) for i in range(n_tasks)]
    w.exemplar_count, w.class_len = 0, []
    w._load_rows({})
    return w


def _extents(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(5, 10, (n,), generator=g), torch.randint(6, 12, (n,), generator=g)], 1)


def test_store_ext_follows_two_truncations():
    """12 rows, 2 classes per task: K/m = 6 -> 3 -> 2.  What manage_memory does on the host (truncate, then the winners' extents
    into the new class blocks) against a list restatement; the frames and target rows move with their extents."""
    w = _host_wrapper(n_mem=4)
    assert tuple(w.store_x.shape) == (12, 1, 9, 11) and tuple(w.store_ext.shape) == (12, 2) and w.store_ext.dtype == torch.int64
    assert w.store_ext.tolist() == [[9, 11]] * 12 and not w.store_ext.is_cuda
    want = [[9, 11] for _ in range(12)]
    blocks = []                                                    # per class: its extents in stored order
    for t, count in enumerate((6, 3, 2)):
        assert count == w.n_total_memories // w.cum_nc_per_task[t]
        w._truncate(count)
        blocks = [b[:count] for b in blocks]
        assert w.exemplar_count == count and w.class_len == [len(b) for b in blocks]
        ext = _extents(2 * count, 60 + t)
        for c in range(2):
            cls = 2 * t + c
            rows = slice(cls * count, (cls + 1) * count)
            w.store_ext[rows] = ext[c * count:(c + 1) * count]
            w.store_x[rows] = torch.arange(count, dtype=torch.float32)[:, None, None, None] + 100 * cls
            w.store_t[rows] = torch.arange(count, dtype=torch.float32)[:, None] + 100 * cls
            blocks.append(ext[c * count:(c + 1) * count].tolist())
        w.class_len.extend([count, count])
        for cls, b in enumerate(blocks):
            want[cls * count:cls * count + len(b)] = b
        assert [w.store_ext[r].tolist() for r in w.stored_rows()] == [e for b in blocks for e in b]
        assert w.store_ext[:len(blocks) * count].tolist() == want[:len(blocks) * count]
    for cls in range(6):                                           # the frames and the targets moved with their extents
        assert w.store_x[2 * cls:2 * cls + 2, 0, 0, 0].tolist() == [100.0 * cls, 100.0 * cls + 1]
        assert w.store_t[2 * cls:2 * cls + 2, 0].tolist() == [100.0 * cls, 100.0 * cls + 1]
    state = w._rows_state()
    assert state["_rows_ext"].tolist() == [e for b in blocks for e in b] and not state["_rows_ext"].is_cuda
    assert tuple(state["_rows_x"].shape) == (12, 1, 9, 11)
    # ... and come back from the pickled rows
    w2 = _host_wrapper(n_mem=4)
    w2.exemplar_count, w2.class_len = 2, [2] * 6
    w2._load_rows(state)
    assert torch.equal(w2.store_ext, w.store_ext) and torch.equal(w2.store_x, w.store_x)


def test_a_state_without_the_new_keys_is_crop_mode():
    from clsurvey_amd.methods.icarl import IcarlNet
    plain = IcarlNet.__new__(IcarlNet)
    assert plain.exemplar_transform is None and plain.frame_shape is None and plain.frame_norm is None and plain.view_seed == 0
    assert plain.last_gather is None and plain.last_exemplar_params is None and plain.last_herd_params is None
    plain.in_shape = (1, 5, 6)
    assert plain.store_shape == (1, 5, 6) and plain.store_dtype == torch.float32
    plain._check_source(None)
    w = _host_wrapper()
    with pytest.raises(ValueError):
        w._check_source(None)


# ---------------------------------------------------------------------------------------------- the two views
def _rng_states():
    return torch.get_rng_state(), np.random.get_state(), random.getstate()


def _same_states(a, b):
    return (torch.equal(a[0], b[0]) and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]
            and a[2] == b[2])


@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized"])
def test_views_are_functions_of_view_seed_and_task_inside_their_own_extents(resized):
    from clsurvey_amd.methods.icarl import VIEW_HERD, VIEW_MEANS, view_seed_of
    w = _host_wrapper(resized=resized)
    ext = _extents(40, 3)
    ext[7] = torch.tensor([5, 6])                                  # no freedom for a plain crop
    torch.manual_seed(1)
    np.random.seed(1)
    random.seed(1)
    before = _rng_states()
    herd = {t: w.view_params(t, VIEW_HERD, ext) for t in range(3)}
    means = {t: w.view_params(t, VIEW_MEANS, ext) for t in range(3)}
    assert _same_states(before, _rng_states())                     # no global generator is touched
    torch.manual_seed(2)                                           # ... nor read
    for t in range(3):
        assert torch.equal(herd[t], w.view_params(t, VIEW_HERD, ext)) and torch.equal(means[t], w.view_params(t, VIEW_MEANS, ext))
        assert torch.equal(herd[t], w.draw_exemplar_params(ext, view_seed_of(0, t, VIEW_HERD)))
        assert not torch.equal(herd[t], means[t])
    assert not torch.equal(herd[0], herd[1]) and not torch.equal(herd[1], herd[2]) and not torch.equal(means[0], means[1])
    w.view_seed = 5
    assert not torch.equal(herd[0], w.view_params(0, VIEW_HERD, ext))
    assert torch.equal(w.view_params(1, VIEW_MEANS, ext), w.draw_exemplar_params(ext, view_seed_of(5, 1, VIEW_MEANS)))
    assert len({view_seed_of(s, t, k) for s in range(4) for t in range(10) for k in (VIEW_HERD, VIEW_MEANS)}) == 80
    for table in list(herd.values()) + list(means.values()):
        p = table.long()
        assert table.dtype == torch.int32 and tuple(table.shape) == (40, 5 if resized else 3) and table.is_contiguous()
        if resized:
            top, left, h, wd, flip = p.unbind(1)
            assert bool((h >= 1).all()) and bool((wd >= 1).all())
        else:
            top, left, flip = p.unbind(1)
            h, wd = torch.full_like(top, 5), torch.full_like(top, 6)
            assert p[7, :2].tolist() == [0, 0]
        assert bool((top >= 0).all()) and bool((top + h <= ext[:, 0]).all())
        assert bool((left >= 0).all()) and bool((left + wd <= ext[:, 1]).all())
        assert bool(((flip == 0) | (flip == 1)).all())
    assert {int(v) for v in herd[0][:, -1]} == {0, 1}


def test_exemplar_draws_with_seeds_are_the_draws_without():
    from clsurvey_amd.methods.icarl import exemplar_draws
    args = (2, 7, [3, 3, 3, 3], 3, [2, 2, 2], [2, 4, 6], 4)
    for seed in (0, 4, 11):
        out = []
        for seeds in (None, []):
            torch.manual_seed(seed)
            np.random.seed(seed)
            random.seed(seed)
            res = exemplar_draws(*args) if seeds is None else exemplar_draws(*args, seeds=seeds)
            out.append((res, _rng_states(), seeds))
        assert out[0][0] == out[1][0] and _same_states(out[0][1], out[1][1])
        counts, plan = out[0][0]
        assert sum(counts) == 7 and [task for task, _ in plan] == [0, 1]
        assert len(out[1][2]) == 2 and all(isinstance(s, int) for s in out[1][2])      # one base seed per past task's loader
    # the replay draws: RehearsalNet.exemplar_params's rule over the rows' own extents
    w = _host_wrapper()
    w.store_ext[:12] = _extents(12, 9)
    gather = [4, 0, 7, 4]
    got = w.exemplar_params(gather, [123, 456])
    assert torch.equal(got, w.draw_exemplar_params(w.store_ext[torch.tensor(gather)], 456)) and tuple(got.shape) == (4, 3)
    assert tuple(w.exemplar_params([], []).shape) == (0, 3)


# ---------------------------------------------------------------------------------------------- icarl_main.main
def _main_args(tmp_path, train, **kw):
    path = os.path.join(str(tmp_path), "SI_first_task.pth.tar")
    with open(path, "wb") as f:
        f.write(b"x")                                              # (must exist; the argument rules come before it is read)
    args = dict(task_name="1", task_count=1, prev_model_path=path, save_path=os.path.join(str(tmp_path), "out"), n_outputs=4,
                method="icarl", postprocess=True, is_scratch_model=True, n_memories=4, n_tasks=2, batch_size=4,
                dataset_path={"train": train, "val": train})
    args.update(kw)
    return args


def test_main_argument_rules_before_a_device_is_needed(tmp_path):
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, RandomResizedCropFlip, TensorTaskDataset
    from clsurvey_amd.methods import icarl_main
    y = torch.arange(8) % 2
    x = torch.zeros((8, 3, 12, 12))
    xb = torch.zeros((8, 3, 12, 12), dtype=torch.uint8)
    mean, std = torch.full((3,), 0.5), torch.full((3,), 0.25)
    names = ["0", "1"]
    plain = TensorTaskDataset(x, y, names)
    crop = TensorTaskDataset(x, y, names, transform=RandomCropFlip((8, 8)))
    resized = TensorTaskDataset(x, y, names, transform=RandomResizedCropFlip((8, 8)))
    bytes_crop = ByteTaskDataset(xb, y, names, mean, std, transform=RandomCropFlip((8, 8)))
    bytes_plain = ByteTaskDataset(xb, y, names, mean, std)

    def run(train, **kw):
        return icarl_main.main(_main_args(tmp_path, train, **kw), [2, 2], device="cpu")
    with pytest.raises(ValueError, match="exemplar_frames=True stores the frames of an augmented train split"):
        run(plain, exemplar_frames=True)
    with pytest.raises(ValueError, match="exemplar_frames=True stores the frames of an augmented train split"):
        run(bytes_plain, exemplar_frames=True, exemplar_dtype="uint8")
    with pytest.raises(NotImplementedError, match="Resized replay is opt-in"):
        run(resized, exemplar_frames=True)
    with pytest.raises(ValueError, match="exemplar_resized=True replays"):
        run(crop, exemplar_frames=True, exemplar_resized=True)
    with pytest.raises(ValueError, match="exemplar_dtype is 'float32' or 'uint8'"):
        run(crop, exemplar_frames=True, exemplar_dtype="float16")
    with pytest.raises(ValueError, match="exemplar_dtype='uint8' stores the byte frames"):
        run(crop, exemplar_frames=True, exemplar_dtype="uint8")
    with pytest.raises(NotImplementedError, match="pass exemplar_dtype='uint8'"):
        run(bytes_crop, exemplar_frames=True)
    # the frame arguments a valid combination gives the wrapper
    ns = types.SimpleNamespace(exemplar_resized=False, exemplar_dtype="uint8")
    frames = icarl_main._frame_arguments(ns, bytes_crop)
    assert frames["exemplar_transform"] is bytes_crop.transform and frames["frame_shape"] == (3, 12, 12)
    assert torch.equal(frames["frame_norm"][0], mean) and torch.equal(frames["frame_norm"][1], std)
    ns = types.SimpleNamespace(exemplar_resized=True, exemplar_dtype="float32")
    assert set(icarl_main._frame_arguments(ns, resized)) == {"exemplar_transform", "frame_shape"}
    # a loaded wrapper whose store kind or mode disagrees with the arguments
    framed = types.SimpleNamespace(exemplar_transform=RandomCropFlip((8, 8)), frame_norm=None)
    icarl_main._check_loaded(framed, dict(exemplar_transform=crop.transform, frame_shape=(3, 12, 12)))
    with pytest.raises(ValueError, match="holds crops"):
        icarl_main._check_loaded(types.SimpleNamespace(exemplar_transform=None), dict(exemplar_transform=crop.transform))
    with pytest.raises(ValueError, match="the loaded wrapper replays"):
        icarl_main._check_loaded(framed, dict(exemplar_transform=resized.transform))
    with pytest.raises(ValueError, match="exemplar store is float32"):
        icarl_main._check_loaded(framed, dict(exemplar_transform=crop.transform, frame_norm=(mean, std)))
