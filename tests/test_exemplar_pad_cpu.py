"""Padded replay of stored exemplars, the parts that need no GPU: the two new entry points and their argument errors, the
exemplar draws of a wrapper with a RandomPadCropFlip spec (draw_pad_crop_flip over the gathered rows' own extents, a function of
the seed, nothing taken from the global generators), the geometry and pad-limit rules of _init_frames, the pickle without the
device fill, and the opt-in switch of gem_main.main, of the method layer and of the driver."""
import ctypes as C
import os
import pickle
import random

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY, ENTRY_U8 = "clhip_rehearsal_assemble_pad_crop_flip", "clhip_rehearsal_assemble_pad_crop_flip_u8"
EINVAL = -1
PAD_MAX, PAD_MAX_EXTENT = 32767, 1 << 30          # CLHIP_PAD_MAX, CLHIP_PAD_MAX_EXTENT (include/clhip.h)


def test_symbols_are_exported_declared_and_in_the_signature_table():
    from clsurvey_amd import _lib
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        header = f.read()
    for entry in (ENTRY, ENTRY_U8):
        assert entry in _lib.SIGNATURES and hasattr(_lib.lib(), entry) and "int %s(" % entry in header
    crop = _lib.SIGNATURES["clhip_rehearsal_assemble_crop_flip"][1]
    pad = _lib.SIGNATURES[ENTRY][1]
    assert pad[:8] == crop[:8] and pad[8:13] == [C.c_int] * 5 and pad[13] == C.c_void_p and pad[14:] == crop[8:]   # mode, 4 pads, fill
    assert len(_lib.SIGNATURES[ENTRY_U8][1]) == len(pad) + 1                                                       # lut
    assert "#define CLHIP_PAD_MAX %d\n" % PAD_MAX in header and "#define CLHIP_PAD_MAX_EXTENT (1 << 30)" in header


@pytest.mark.parametrize("entry", [ENTRY, ENTRY_U8])
def test_argument_errors_do_not_need_a_device(entry):
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = getattr(_lib.lib(), entry)
    u8 = entry == ENTRY_U8

    def call(x=one, y=one, B=4, geo=(3, 20, 20, 16, 16), mode=2, pads=(4, 4, 4, 4), fill=one, lut=one, src=one, src_rows=9,
             src_idx=one, store=one, store_y=one, store_rows=12, row0=2, ring=3, gather=one, params=one, E=2, x_mix=one, y_mix=one):
        table = (lut,) if u8 else ()
        return f(x, y, B, *geo, mode, *pads, fill, *table, src, src_rows, src_idx, store, store_y, store_rows, row0, ring, gather,
                 params, E, x_mix, y_mix, None)
    # what clhip_rehearsal_assemble_crop_flip refuses
    assert call(B=-1) == EINVAL and call(E=-1) == EINVAL and call(ring=-1) == EINVAL and call(store_rows=-1) == EINVAL
    assert call(ring=5) == EINVAL                                 # ring rows are a prefix of the batch
    assert call(x=None) == EINVAL and call(y=None) == EINVAL and call(y_mix=None) == EINVAL
    assert call(store=None) == EINVAL and call(store_y=None) == EINVAL and call(gather=None) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=10) == EINVAL
    assert call(B=70000, ring=0) == EINVAL
    for geo in ((0, 20, 20, 16, 16), (3, 0, 20, 16, 16), (3, 20, 0, 16, 16), (3, 20, 20, 0, 16), (3, 20, 20, 16, 0), (3, 20, 20, -1, 16)):
        assert call(geo=geo) == EINVAL, geo
    assert call(params=None) == EINVAL and call(src=None) == EINVAL and call(src_idx=None) == EINVAL and call(src_rows=-1) == EINVAL
    assert call(x_mix=None) == EINVAL                             # x_mix may be missing only without exemplars
    # the padding
    for mode in (-1, 4, 100):
        assert call(mode=mode) == EINVAL, mode
    for k in range(4):
        for v in (-1, PAD_MAX + 1):
            pads = [4, 4, 4, 4]
            pads[k] = v
            assert call(pads=pads) == EINVAL, pads
    assert call(geo=(3, PAD_MAX_EXTENT + 1, 20, 16, 16)) == EINVAL and call(geo=(3, 20, PAD_MAX_EXTENT + 1, 16, 16)) == EINVAL
    assert call(fill=None) == EINVAL and call(fill=None, B=0, ring=0, E=1) == EINVAL      # the fill: needed exactly with exemplars
    # ... and every one of them also where nothing would be launched
    assert call(mode=4, B=0, ring=0, E=0) == EINVAL and call(pads=(0, -1, 0, 0), B=0, ring=0, E=0) == EINVAL
    # legal and without work: no launch, no device
    assert call(B=0, ring=0, E=0) == 0                            # nothing to do
    assert call(B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0    # the ring-only form with an empty ring
    assert call(B=4, ring=0, E=0, x_mix=None, y_mix=None, fill=None, lut=None) == 0      # ... which needs neither fill nor table
    assert call(fill=None, B=0, ring=0, E=0) == 0
    for mode in range(4):
        assert call(mode=mode, pads=(PAD_MAX, 0, PAD_MAX, 0), B=0, ring=0, E=0) == 0
    # a crop larger than the frame is legal here: the padded image may hold it (the crop entry refuses it)
    assert call(geo=(3, 8, 8, 12, 12), B=0, ring=0, E=0) == 0
    crop = getattr(_lib.lib(), "clhip_rehearsal_assemble_crop_flip" + ("_u8" if u8 else ""))
    assert crop(one, one, 0, 3, 8, 8, 12, 12, *((one,) if u8 else ()), one, 9, one, one, one, 12, 2, 0, one, one, 0, one, one, None) == EINVAL
    if u8:                                                        # the table: needed exactly when exemplars are decoded
        assert call(lut=None) == EINVAL and call(lut=None, B=0, ring=0, E=1) == EINVAL
        assert call(lut=None, B=0, ring=0, E=0) == 0


def test_ops_refuse_cpu_tensors_and_check_the_table():
    from clsurvey_amd import ops
    geo = (3, 8, 8, 12, 12)
    store, store_y = torch.zeros((4,) + geo[:3]), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device tensors"):
        ops.rehearsal_assemble_pad_crop_flip(geo, "reflect", (2, 2, 2, 2), torch.zeros(3), None, store_y, 2, store, store_y, store,
                                             store_y, 0, 2, None, None, None, None)
    with pytest.raises(RuntimeError, match="HIP device tensors"):
        ops.rehearsal_assemble_pad_crop_flip_u8(geo, 0, (2, 2, 2, 2), torch.zeros(3), torch.zeros((3, 256)), None, store_y, 2,
                                                store.byte(), store_y, store.byte(), store_y, 0, 2, None, None, None, None)


# ---------------------------------------------------------------------------------------------- the host side of a wrapper
FRAME, CROP, PADS = (1, 9, 11), (10, 12), (2, 1, 3, 2)            # the crop is larger than the frame; pads (left, top, right, bottom)


def _spec(padding=PADS, **kw):
    from clsurvey_amd.data import RandomPadCropFlip
    return RandomPadCropFlip(CROP, padding, **kw)


def _host_wrapper(spec=None, full=False, n_tasks=3, n_mem=6, frame=FRAME, frame_norm=None):
    """A RehearsalNet without net and engine: the host side of the store (as test_exemplar_resized_cpu._host_wrapper)."""
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.device = torch.device("cpu")
    w.in_shape = (frame[0],) + CROP
    w._init_frames(_spec() if spec is None else spec, frame, frame_norm)
    w.full_mem_mode, w.n_tasks, w.n_total_memories = full, n_tasks, n_mem * n_tasks
    w.n_memories = w.n_total_memories if full else n_mem
    w.observed_tasks, w.old_task, w.mem_cnt, w.filled = [], -1, 0, [0] * n_tasks
    w.n_append, w.chunk_size = 0, 4
    w._load_rows({})
    return w


def test_init_frames_keeps_the_spec_without_its_extents():
    from clsurvey_amd.data import RandomPadCropFlip
    spec = _spec(fill=0.25, padding_mode="symmetric", p=0.25, extents=torch.tensor([[9, 11]] * 4))
    w = _host_wrapper(spec)
    t = w.exemplar_transform
    assert isinstance(t, RandomPadCropFlip) and t is not spec and t.extents is None
    assert (t.size, t.padding, t.fill, t.padding_mode, t.p) == (CROP, PADS, 0.25, "symmetric", 0.25)
    assert w.frame_shape == FRAME and w.store_shape == FRAME and w.geometry == FRAME + CROP and w.params_width == 5
    assert tuple(w.store_x.shape) == (18,) + FRAME and w.store_ext.tolist() == [[9, 11]] * 18
    assert w.fill is None                                         # the device vector is _bind's


def test_init_frames_asks_that_the_padded_frame_holds_the_crop_and_checks_the_modes_limit():
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.in_shape = (1,) + CROP
    with pytest.raises(ValueError, match="frames"):
        w._init_frames(_spec(), (1, 6, 11))                       # 6 + 1 + 2 < 10
    with pytest.raises(ValueError, match="frames"):
        w._init_frames(_spec(), (1, 9, 6))                        # 6 + 2 + 3 < 12
    with pytest.raises(ValueError, match="frames"):
        w._init_frames(_spec(), (2, 9, 11))                       # another channel count
    with pytest.raises(TypeError):
        w._init_frames(_spec(), None)
    w._init_frames(_spec(), (1, 7, 7))                            # 7 + 3 = 10, 7 + 5 = 12: exactly held
    assert w.frame_shape == (1, 7, 7)
    # reflect takes pads up to extent - 1, symmetric up to extent
    w._init_frames(_spec((5, 3, 5, 3), padding_mode="symmetric"), (1, 9, 5))
    with pytest.raises(ValueError, match="padding_mode 'reflect' takes pads up to the extent - 1"):
        w._init_frames(_spec((5, 3, 5, 3), padding_mode="reflect"), (1, 9, 5))
    w._init_frames(_spec((4, 3, 4, 3), padding_mode="reflect"), (1, 9, 5))
    with pytest.raises(ValueError, match="padding_mode 'symmetric' takes pads up to the extent,"):
        w._init_frames(_spec((0, 1, 0, 5), padding_mode="symmetric"), (1, 4, 12))
    for mode in ("constant", "edge"):
        w._init_frames(_spec((20, 20, 20, 20), padding_mode=mode), (1, 2, 2))
    # the fill: one value per channel, bytes on a byte store
    with pytest.raises(ValueError, match="fill values for"):
        w._init_frames(_spec(fill=(0.0, 1.0)), FRAME)
    with pytest.raises(ValueError, match="ints in 0..255"):
        w._init_frames(_spec(fill=0.5), FRAME, ([0.5], [0.25]))
    w._init_frames(_spec(fill=128), FRAME, ([0.5], [0.25]))
    assert w.store_dtype == torch.uint8


def _filled_wrapper(spec=None):
    w = _host_wrapper(spec)
    w.observed_tasks, w.old_task, w.filled = [0, 1, 2], 2, [6, 6, 0]
    w.n_append, w.chunk_size = 7, 3
    g = torch.Generator().manual_seed(1)
    w.store_ext[:12] = torch.stack([torch.randint(7, 10, (12,), generator=g), torch.randint(7, 12, (12,), generator=g)], 1)
    return w


def _planned(w, seed):
    random.seed(seed)
    torch.manual_seed(seed)
    seeds = []
    _, plan = w.plan(2, seeds)
    gather = [w._row(past, s) for past, _, chs in plan for ch in chs for s in ch]
    return gather, w.exemplar_params(gather, seeds), seeds, torch.get_rng_state(), random.getstate()


def test_exemplar_draws_are_draw_pad_crop_flip_over_the_gathered_rows_own_extents():
    from clsurvey_amd.data import RandomPadCropFlip, draw_pad_crop_flip
    w = _filled_wrapper()
    pl, pt, pr, pb = PADS
    seen = set()
    for seed in range(30):
        gather, params, seeds, _, _ = _planned(w, seed)
        again = _planned(w, seed)
        assert len(gather) == 7 and again[0] == gather and torch.equal(again[1], params)
        assert params.dtype == torch.int32 and tuple(params.shape) == (7, 5) and params.is_contiguous()
        ext = w.store_ext[torch.tensor(gather)]
        assert torch.equal(params, w.draw_exemplar_params(ext, seeds[-1]))
        want = draw_pad_crop_flip(7, RandomPadCropFlip(CROP, PADS, extents=ext), FRAME[1:], torch.Generator().manual_seed(seeds[-1]))
        assert torch.equal(params, want)
        p = params.long()
        assert torch.equal(p[:, 3:], ext)                          # (h, w): the stored frame's own extent
        assert bool((p[:, 0] >= -pt).all()) and bool((p[:, 0] <= ext[:, 0] + pb - CROP[0]).all())
        assert bool((p[:, 1] >= -pl).all()) and bool((p[:, 1] <= ext[:, 1] + pr - CROP[1]).all())
        assert bool(((p[:, 2] == 0) | (p[:, 2] == 1)).all())
        seen.update(map(tuple, p.tolist()))
    assert len(seen) > 40 and {r[2] for r in seen} == {0, 1} and min(r[0] for r in seen) < 0 and min(r[1] for r in seen) < 0


def test_with_all_pads_zero_the_draws_are_the_crop_specs():
    """draw_pad_crop_flip's i is draw_crop_flip's top on the padded extent; with pads 0 the first three columns are the
    RandomCropFlip wrapper's draws for the same seed, the last two the extents."""
    from clsurvey_amd.data import RandomCropFlip, RandomPadCropFlip
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    frame, crop = (1, 9, 11), (5, 6)
    ws = []
    for spec in (RandomPadCropFlip(crop, 0, p=0.3), RandomCropFlip(crop, 0.3)):
        w = RehearsalNet.__new__(RehearsalNet)
        w.in_shape = (1,) + crop
        w._init_frames(spec, frame)
        ws.append(w)
    g = torch.Generator().manual_seed(4)
    ext = torch.stack([torch.randint(5, 10, (40,), generator=g), torch.randint(6, 12, (40,), generator=g)], 1)
    for seed in (0, 3, 2 ** 40 + 5):
        a, b = ws[0].draw_exemplar_params(ext, seed), ws[1].draw_exemplar_params(ext, seed)
        assert tuple(a.shape) == (40, 5) and tuple(b.shape) == (40, 3)
        assert torch.equal(a[:, :3], b) and torch.equal(a[:, 3:].long(), ext)
    assert len({tuple(r) for r in a[:, :3].tolist()}) > 20


def test_the_draws_leave_the_global_generators_alone():
    """The plan consumes the generators as the crop spec's does; the draws themselves take nothing."""
    from clsurvey_amd.data import RandomCropFlip
    a, b = _filled_wrapper(), _filled_wrapper()
    b.exemplar_transform = RandomCropFlip((5, 6), 0.5)
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


def test_draws_refuse_an_extent_the_mode_cannot_pad():
    """The limit is checked against the frame at construction and against the gathered rows' own extents at every draw."""
    w = _filled_wrapper(_spec((5, 3, 5, 3), padding_mode="reflect"))
    w.store_ext[4] = torch.tensor([9, 5])                         # 5 + 10 holds the crop, but reflect takes pads up to 4 here
    w.draw_exemplar_params(w.store_ext[:4], 5)
    with pytest.raises(ValueError, match="padding_mode 'reflect'"):
        w.draw_exemplar_params(w.store_ext[:6], 5)


# ---------------------------------------------------------------------------------------------- the pickle
def test_the_wrapper_pickles_without_its_device_fill():
    from clsurvey_amd.data import RandomPadCropFlip
    from clsurvey_amd.methods.exemplar import ExemplarNet
    from clsurvey_amd.methods.gem import GemNet
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    assert "fill" in ExemplarNet._TRANSIENT and "lut" in ExemplarNet._TRANSIENT and ExemplarNet.fill is None
    for cls in (RehearsalNet, GemNet):
        w = _host_wrapper(_spec(fill=0.5, padding_mode="edge"))
        w.__class__ = cls
        w.fill = torch.tensor([0.5])                              # what _bind leaves
        w.memory_x = w.memory_labels = w.memory_ext = None
        state = w.__getstate__()
        assert "fill" not in state and "lut" not in state
        t = pickle.loads(pickle.dumps(state["exemplar_transform"]))
        assert isinstance(t, RandomPadCropFlip) and (t.size, t.padding, t.fill, t.padding_mode) == (CROP, PADS, 0.5, "edge")
        assert state["frame_shape"] == FRAME


# ---------------------------------------------------------------------------------------------- the switch
def _args(root, method, train, val, **kw):
    prev = os.path.join(root, "prev.pth.tar")
    torch.save({}, prev)
    return dict(task_name="2", task_count=2, prev_model_path=prev, n_outputs=4, method=method, n_memories=4, n_tasks=2,
                dataset_path={"train": train, "val": val, "test": val}, postprocess=False, is_scratch_model=False, **kw)


def _padded_split(byte=False):
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip, TensorTaskDataset
    y = torch.arange(8) % 2
    if byte:
        return ByteTaskDataset(torch.zeros((8, 3, 12, 12), dtype=torch.uint8), y, ["0", "1"], [0.5] * 3, [0.25] * 3,
                               transform=RandomPadCropFlip((12, 12), 2, fill=128))
    return TensorTaskDataset(torch.zeros((8, 3, 12, 12)), y, ["0", "1"], transform=RandomPadCropFlip((12, 12), 2))


METHODS = ["gem", "baseline_rehearsal_full_mem", "baseline_rehearsal_partial_mem"]


@pytest.mark.parametrize("method", METHODS)
def test_without_the_switch_the_entry_still_refuses(tmp_path, method):
    from clsurvey_amd.methods import gem_main
    for byte, extra in ((False, {}), (False, dict(exemplar_padded=False)), (True, dict(exemplar_dtype="uint8")),
                        (False, dict(exemplar_resized=True))):
        train = _padded_split(byte)
        with pytest.raises(NotImplementedError, match="padded replay is not built"):
            gem_main.main(_args(str(tmp_path), method, train, train, **extra), [2, 2], device="cpu")


@pytest.mark.parametrize("method", METHODS)
def test_with_the_switch_the_refusal_is_gone(tmp_path, method):
    """The entry gets past every check made on the split alone and as far as a CPU device goes: the prev_model_path of these
    arguments holds an empty dict, not a wrapper, and that is what stops it."""
    from clsurvey_amd.methods import gem_main
    for byte in (False, True):
        train = _padded_split(byte)
        extra = dict(exemplar_dtype="uint8") if byte else {}
        with pytest.raises(AttributeError, match="'dict' object has no attribute 'batch_size'"):
            gem_main.main(_args(str(tmp_path), method, train, train, exemplar_padded=True, **extra), [2, 2], device="cpu")


@pytest.mark.parametrize("method", METHODS)
def test_the_switch_belongs_to_a_padded_split_and_keeps_the_byte_rules(tmp_path, method):
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, RandomResizedCropFlip, TensorTaskDataset
    from clsurvey_amd.methods import gem_main
    x, y = torch.zeros((4, 3, 16, 16)), torch.tensor([0, 1, 0, 1])
    plain = TensorTaskDataset(x[:, :, :8, :8], y, list("ab"))
    crop = TensorTaskDataset(x, y, list("ab"), transform=RandomCropFlip((8, 8)))
    resized = TensorTaskDataset(x, y, list("ab"), transform=RandomResizedCropFlip((8, 8)))
    for train in (crop, plain, resized):
        with pytest.raises(ValueError, match="exemplar_padded=True replays the exemplars through the RandomPadCropFlip"):
            gem_main.main(_args(str(tmp_path), method, train, plain, exemplar_padded=True), [2, 2], device="cpu")
    # the padded spec is treated like the other two by the byte rules
    with pytest.raises(ValueError, match="exemplar_dtype='uint8'.*ByteTaskDataset carrying a RandomCropFlip"):
        gem_main.main(_args(str(tmp_path), method, _padded_split(), plain, exemplar_padded=True, exemplar_dtype="uint8"), [2, 2], device="cpu")
    with pytest.raises(NotImplementedError, match="byte frames.*exemplar_dtype='uint8'"):
        gem_main.main(_args(str(tmp_path), method, _padded_split(True), plain, exemplar_padded=True), [2, 2], device="cpu")
    # both opt-ins at once: a split carries one transform
    with pytest.raises(ValueError, match="exemplar_resized=True"):
        gem_main.main(_args(str(tmp_path), method, _padded_split(), plain, exemplar_padded=True, exemplar_resized=True), [2, 2], device="cpu")
    assert isinstance(_padded_split(True), ByteTaskDataset)


def test_icarl_refuses_in_every_combination(tmp_path):
    from clsurvey_amd.methods import icarl_main
    path = os.path.join(str(tmp_path), "SI_first_task.pth.tar")
    with open(path, "wb") as f:
        f.write(b"x")                                              # (must exist; the refusal comes before it is read)
    for byte, extra in ((False, dict(exemplar_padded=True)), (False, dict(exemplar_frames=True, exemplar_padded=True)),
                        (True, dict(exemplar_frames=True, exemplar_dtype="uint8", exemplar_padded=True)),
                        (False, dict(exemplar_frames=True, exemplar_resized=True, exemplar_padded=True))):
        train = _padded_split(byte)
        args = dict(task_name="1", task_count=1, prev_model_path=path, save_path=os.path.join(str(tmp_path), "out"), n_outputs=4,
                    method="icarl", postprocess=True, is_scratch_model=True, n_memories=4, n_tasks=2, batch_size=4,
                    dataset_path={"train": train, "val": train}, **extra)
        with pytest.raises(NotImplementedError, match="padded replay is not built"):
            icarl_main.main(args, [2, 2], device="cpu")


# ---------------------------------------------------------------------------------------------- method layer and driver
def test_the_method_layer_sets_the_argument_only_when_given(monkeypatch):
    """--padded_exemplars reaches gem_main.main as exemplar_padded=True for GEM and the rehearsal baselines, never for iCaRL, and
    without the flag the recorded trainer arguments are what they were."""
    import types
    from clsurvey_amd.methods import method as M
    seen = []
    monkeypatch.setattr(M._gem, "main", lambda kw, nc, device=None: seen.append(("gem", dict(kw))))
    monkeypatch.setattr(M._icarl, "main", lambda kw, nc, device=None: seen.append(("icarl", dict(kw))))

    class _Dataset:
        task_count = 2
        classes_per_task = {"1": ["a", "b"], "2": ["c", "d"]}

    def manager():
        return types.SimpleNamespace(dataset=_Dataset(), previous_task_model_path="prev", current_task_dataset_path="data",
                                     gridsearch_exp_dir="exp", overwrite_args=None)

    def args(**kw):
        return types.SimpleNamespace(task_counter=2, task_name="2", mem_per_task=4, num_epochs=1, batch_size=8, device="cpu",
                                     weight_decay=0.0, lr=0.01, **kw)
    for flags in ({}, {"padded_exemplars": True}):
        seen.clear()
        M._gem_run(M.parse("GEM"), args(**flags), manager(), 0.5, "out")
        M._rehearsal_grid_train(M.parse("finetuning_rehearsal_partial_mem"), args(**flags), manager(), 0.01)
        M._icarl_run(M.parse("ICARL"), args(**flags), manager(), 1.0, "out")
        assert [k for k, _ in seen] == ["gem", "gem", "icarl"]
        for _, kw in seen[:2]:
            assert kw.get("exemplar_padded", None) == (True if flags else None)
            assert ("exemplar_padded" in kw) == bool(flags)
        assert "exemplar_padded" not in seen[2][1]


def test_driver_flag_checks(tmp_path):
    from clsurvey_amd.framework import driver
    argv = ["small_VGG9_cl_128_128", "--results_root", str(tmp_path), "--synthetic", "2,4,16,8,8,32", "--method_name",
            "finetuning_rehearsal_partial_mem", "--mem_per_task", "4"]
    for extra in ([], ["--rnd_margin", "4"], ["--rnd_resized", "4", "--resized_exemplars"]):
        with pytest.raises(SystemExit, match="--padded_exemplars belongs with --rnd_pad"):
            driver.main(argv + ["--padded_exemplars"] + extra)
    # a byte store on padded tasks needs both switches, and byte frames
    with pytest.raises(SystemExit, match="--u8_exemplars belongs with"):
        driver.main(argv + ["--rnd_pad", "2", "--u8_frames", "--u8_exemplars"])
    with pytest.raises(SystemExit, match="--u8_exemplars belongs with"):
        driver.main(argv + ["--rnd_pad", "2", "--padded_exemplars", "--u8_exemplars"])
    assert not os.path.exists(os.path.join(str(tmp_path), "data"))                   # raised before anything is generated
    p = driver.build_parser()
    assert p.parse_args(argv + ["--rnd_pad", "2", "--padded_exemplars"]).padded_exemplars is True
    assert p.parse_args(argv).padded_exemplars is False
