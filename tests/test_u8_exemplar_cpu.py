"""The byte exemplar store, the parts that need no GPU: the new entry point and its argument errors, the opt-in switch of
gem_main.main, and the host side of a byte-store wrapper (which batches it takes, how a state without frame_norm loads)."""
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
ENTRY = "clhip_rehearsal_assemble_crop_flip_u8"


def test_symbol_is_exported_declared_and_in_the_signature_table():
    from clsurvey_amd import _lib
    assert ENTRY in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[ENTRY][1]) == len(_lib.SIGNATURES["clhip_rehearsal_assemble_crop_flip"][1]) + 1        # lut
    assert hasattr(_lib.lib(), ENTRY)
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        assert "int %s(" % ENTRY in f.read()


def test_argument_errors_do_not_need_a_device():
    import ctypes as C
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = getattr(_lib.lib(), ENTRY)

    def call(x=one, y=one, B=4, geo=(3, 20, 20, 16, 16), lut=one, src=one, src_rows=9, src_idx=one, store=one, store_y=one,
             store_rows=12, row0=2, ring=3, gather=one, params=one, E=2, x_mix=one, y_mix=one):
        return f(x, y, B, *geo, lut, src, src_rows, src_idx, store, store_y, store_rows, row0, ring, gather, params, E, x_mix, y_mix,
                 None)
    # the fp32 entry's cases
    assert call(B=-1) == -1 and call(E=-1) == -1 and call(ring=-1) == -1 and call(store_rows=-1) == -1
    assert call(ring=5) == -1                                     # ring rows are a prefix of the batch
    assert call(x=None) == -1 and call(y=None) == -1 and call(y_mix=None) == -1
    assert call(store=None) == -1 and call(store_y=None) == -1 and call(gather=None) == -1
    assert call(row0=-1) == -1 and call(row0=10) == -1
    assert call(B=70000, ring=0) == -1
    for geo in ((0, 20, 20, 16, 16), (3, 20, 20, 21, 16), (3, 20, 20, 16, 21), (3, 20, 20, 0, 16), (3, 20, 20, 16, 0)):
        assert call(geo=geo) == -1, geo
    assert call(params=None) == -1 and call(src=None) == -1 and call(src_idx=None) == -1 and call(src_rows=-1) == -1
    assert call(x_mix=None) == -1                                 # x_mix may be missing only without exemplars
    assert call(B=0, ring=0, E=0) == 0                            # nothing to do
    assert call(B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0    # the ring-only form with an empty ring
    # the table: needed exactly when exemplars are decoded
    assert call(lut=None) == -1
    assert call(lut=None, B=0, ring=0, E=1) == -1
    assert call(lut=None, B=4, ring=0, E=0, x_mix=None, y_mix=None) == 0
    assert call(lut=None, B=0, ring=0, E=0) == 0


# ---------------------------------------------------------------------------------------------- gem_main.main
def _frames():
    return torch.randint(0, 256, (4, 3, 16, 16), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)


def _args(root, method, train, val):
    prev = os.path.join(root, "prev.pth.tar")
    torch.save({}, prev)
    return dict(task_name="2", task_count=2, prev_model_path=prev, n_outputs=8, method=method, n_memories=4, n_tasks=2,
                dataset_path={"train": train, "val": val, "test": val}, postprocess=False, is_scratch_model=False)


@pytest.mark.parametrize("method", ["gem", "baseline_rehearsal_full_mem", "baseline_rehearsal_partial_mem"])
def test_uint8_exemplars_need_an_augmented_byte_split(tmp_path, method):
    """exemplar_dtype='uint8' on a byte split without a transform, and on a float split with one: a ValueError that says so,
    raised before any loader or device is touched.  Any other value of the argument is a ValueError too."""
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip
    from clsurvey_amd.methods import gem_main
    x, y = _frames(), torch.tensor([0, 1, 2, 3])
    plain = ByteTaskDataset(x[:, :, :8, :8], y, list("abcd"), *IMAGENET)
    floats = ByteTaskDataset(x, y, list("abcd"), *IMAGENET, transform=RandomCropFlip((8, 8))).decoded()
    for train in (plain, floats):
        args = dict(_args(str(tmp_path), method, train, plain), exemplar_dtype="uint8")
        with pytest.raises(ValueError, match="exemplar_dtype='uint8'.*ByteTaskDataset carrying a RandomCropFlip"):
            gem_main.main(args, [4, 4], device="cpu")
    with pytest.raises(ValueError, match="exemplar_dtype"):
        gem_main.main(dict(_args(str(tmp_path), method, plain, plain), exemplar_dtype="float16"), [4, 4], device="cpu")


def test_the_default_still_refuses_and_names_the_switch(tmp_path):
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, RandomResizedCropFlip
    from clsurvey_amd.methods import gem_main
    x, y = _frames(), torch.tensor([0, 1, 2, 3])
    plain = ByteTaskDataset(x[:, :, :8, :8], y, list("abcd"), *IMAGENET)
    aug = ByteTaskDataset(x, y, list("abcd"), *IMAGENET, transform=RandomCropFlip((8, 8)))
    for extra in ({}, {"exemplar_dtype": "float32"}):
        with pytest.raises(NotImplementedError, match="byte frames.*exemplar_dtype='uint8'"):
            gem_main.main(dict(_args(str(tmp_path), "gem", aug, plain), **extra), [4, 4], device="cpu")
    # the resized spec's refusal comes first, with or without the switch
    resized = ByteTaskDataset(x, y, list("abcd"), *IMAGENET, transform=RandomResizedCropFlip((8, 8)))
    for extra in ({}, {"exemplar_dtype": "uint8"}):
        with pytest.raises(NotImplementedError, match="RandomCropFlip only"):
            gem_main.main(dict(_args(str(tmp_path), "gem", resized, plain), **extra), [4, 4], device="cpu")


# ---------------------------------------------------------------------------------------------- the host side of a wrapper
FRAME, CROP = (3, 9, 11), (5, 6)


def _host_wrapper(frame_norm, n_tasks=3, n_mem=6):
    """A RehearsalNet without net and engine: the host side of the store (as test_exemplar_augment_cpu._host_wrapper)."""
    from clsurvey_amd.data import RandomCropFlip
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    w = RehearsalNet.__new__(RehearsalNet)
    w.device = torch.device("cpu")
    w.in_shape = (FRAME[0],) + CROP
    w._init_frames(RandomCropFlip(CROP, 0.5), FRAME, frame_norm)
    w.full_mem_mode, w.n_tasks, w.n_total_memories = False, n_tasks, n_mem * n_tasks
    w.n_memories = n_mem
    w.observed_tasks, w.old_task, w.mem_cnt, w.filled = [], -1, 0, [0] * n_tasks
    w.n_append, w.chunk_size = 0, 4
    w._load_rows({})
    return w


def _source(dtype, norm):
    from clsurvey_amd.methods.exemplar import BatchSource
    idx = torch.tensor([0, 1], dtype=torch.int64)
    return BatchSource(torch.zeros((10,) + FRAME, dtype=dtype), idx, idx, None, norm)


def test_batch_source_keeps_its_four_argument_form():
    from clsurvey_amd.methods.exemplar import BatchSource
    idx = torch.tensor([0])
    assert BatchSource(torch.zeros(1), idx, idx, None).norm is None
    assert BatchSource._fields == ("frames", "idx", "idx_host", "extents", "norm")


def test_a_byte_store_is_uint8_and_keeps_its_norm_on_the_host():
    w = _host_wrapper(IMAGENET)
    assert w.store_x.dtype == torch.uint8 and tuple(w.store_x.shape) == (18,) + FRAME and w.store_dtype == torch.uint8
    mean, std = w.frame_norm
    assert mean.dtype == std.dtype == torch.float32 and not mean.is_cuda and not std.is_cuda
    assert torch.equal(mean, torch.tensor(IMAGENET[0])) and torch.equal(std, torch.tensor(IMAGENET[1]))
    state = w.__getstate__()
    assert "lut" not in state and state["frame_norm"] is w.frame_norm and state["_rows_x"].dtype == torch.uint8
    f = _host_wrapper(None)
    assert f.store_x.dtype == torch.float32 and f.frame_norm is None and f.store_dtype == torch.float32
    with pytest.raises(ValueError):
        _host_wrapper(((0.5, 0.5), (0.2, 0.2)))                   # two values for three channels


def test_check_source_refuses_the_other_kind_of_frames():
    norm = tuple(torch.tensor(v) for v in IMAGENET)
    byte, flt = _host_wrapper(IMAGENET), _host_wrapper(None)
    byte._check_source(_source(torch.uint8, norm))
    flt._check_source(_source(torch.float32, None))
    with pytest.raises(ValueError, match="uint8 store"):
        byte._check_source(_source(torch.float32, None))          # float frames for a byte store
    with pytest.raises(ValueError, match="uint8 store"):
        byte._check_source(_source(torch.uint8, None))            # bytes that do not say what they mean
    with pytest.raises(ValueError, match="float32 store"):
        flt._check_source(_source(torch.uint8, norm))             # the reverse
    with pytest.raises(ValueError):
        byte._check_source(None)


def test_check_source_refuses_another_mean_or_std():
    byte = _host_wrapper(IMAGENET)
    mean, std = (torch.tensor(v) for v in IMAGENET)
    other_mean, other_std = mean.clone(), std.clone()
    other_mean[2] = 0.407
    other_std[0] = 0.2291
    byte._check_source(_source(torch.uint8, (mean.clone(), std.clone())))
    for norm in ((other_mean, std), (mean, other_std)):
        with pytest.raises(ValueError, match="one table decodes"):
            byte._check_source(_source(torch.uint8, norm))


def test_a_state_without_frame_norm_loads_as_an_fp32_wrapper():
    """What a frame-mode wrapper pickled before the byte store existed looks like."""
    from clsurvey_amd.methods.gem import GemNet
    from clsurvey_amd.methods.rehearsal import RehearsalNet
    assert RehearsalNet.frame_norm is None and GemNet.frame_norm is None and RehearsalNet.lut is None
    w = _host_wrapper(IMAGENET)
    state = {k: v for k, v in w.__dict__.items() if k not in ("store_x", "store_y", "store_ext")}
    assert "frame_norm" in state
    del state["frame_norm"]
    old = RehearsalNet.__new__(RehearsalNet)
    old.__dict__.update(state)
    old._load_rows({})
    assert old.frame_norm is None and old.store_dtype == torch.float32 and old.store_x.dtype == torch.float32
    assert old.exemplar_transform is not None and old.frame_shape == FRAME
    old._check_source(_source(torch.float32, None))
