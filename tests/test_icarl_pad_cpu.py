"""iCaRL on padded RandomCrop tasks, the parts that need no GPU: the two padded step-assembly entries and their argument errors,
the argument rules of icarl_main.main for exemplar_pad_frames that are decided before a device is needed, the method layer's and
the driver's switch, and IcarlNet's dispatch to the padded ops."""
import os
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ["clhip_icarl_assemble_pad_crop_flip", "clhip_icarl_assemble_pad_crop_flip_u8"]
PAD_MAX, PAD_MAX_EXTENT = 32767, 1 << 30                           # CLHIP_PAD_MAX, CLHIP_PAD_MAX_EXTENT (include/clhip.h)


def test_symbols_are_exported_and_declared():
    from clsurvey_amd import _lib, ops
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        header = f.read()
    assert "#define CLHIP_PAD_MAX %d" % PAD_MAX in header and "#define CLHIP_PAD_MAX_EXTENT (1 << 30)" in header
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
        assert "int %s(" % name in header
        assert callable(getattr(ops, name[len("clhip_"):]))
    crop = _lib.SIGNATURES["clhip_icarl_assemble_crop_flip"][1]
    for name in ENTRIES:                                           # mode, four pads and fill go behind the geometry
        want = crop[:8] + [crop[2]] * 5 + [crop[0]] + (crop[8:9] if name.endswith("_u8") else []) + crop[8:]
        assert _lib.SIGNATURES[name][1] == want


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_do_not_need_a_device(entry):
    import ctypes as C
    from clsurvey_amd import _lib
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    # (every call below is refused, or has B = E = 0: none reaches a launch, with or without a device)
    f = getattr(_lib.lib(), entry)
    u8 = entry.endswith("_u8")

    def call(x=one, y=one, B=4, geo=(3, 20, 20, 16, 16), mode=2, pads=(4, 4, 4, 4), fill=one, lut=one, store=one, store_rows=12,
             gather=one, params=one, E=2, store_t=one, n_outputs=12, x_mix=one, y_mix=one, t_mix=one):
        table = (lut,) if u8 else ()
        return f(x, y, B, *geo, mode, *pads, fill, *table, store, store_rows, gather, params, E, store_t, n_outputs, x_mix, y_mix,
                 t_mix, None)
    EINVAL = -1
    assert call(B=-1) == EINVAL and call(E=-1) == EINVAL and call(store_rows=-1) == EINVAL              # negative counts
    for geo in ((0, 20, 20, 16, 16), (3, 0, 20, 16, 16), (3, 20, 0, 16, 16), (3, 20, 20, 0, 16), (3, 20, 20, 16, 0)):
        assert call(geo=geo) == EINVAL, geo
    assert call(n_outputs=0) == EINVAL and call(n_outputs=-4) == EINVAL
    for geo in ((3, 20, 20, 28, 16), (3, 20, 20, 16, 28), (3, 8, 8, 12, 12)):     # a padded image may hold a crop larger than the frame
        assert call(geo=geo, B=0, E=0) == 0, geo
    for geo in ((3, PAD_MAX_EXTENT + 1, 20, 16, 16), (3, 20, PAD_MAX_EXTENT + 1, 16, 16)):
        assert call(geo=geo) == EINVAL and call(geo=geo, B=0, E=0) == EINVAL, geo
    assert call(geo=(3, PAD_MAX_EXTENT, PAD_MAX_EXTENT, 16, 16), B=0, E=0) == 0
    for mode in (-1, 4, 17):
        assert call(mode=mode) == EINVAL and call(mode=mode, B=0, E=0) == EINVAL, mode
    for mode in (0, 1, 2, 3):
        assert call(mode=mode, B=0, E=0) == 0
    for k in range(4):
        for v in (-1, PAD_MAX + 1):
            pads = tuple(v if i == k else 4 for i in range(4))
            assert call(pads=pads) == EINVAL and call(pads=pads, B=0, E=0) == EINVAL, pads
    assert call(pads=(PAD_MAX, 0, PAD_MAX, 0), B=0, E=0) == 0
    # missing pointers for a non-zero count
    for name in ("x", "y", "x_mix", "y_mix"):
        assert call(**{name: None}) == EINVAL, name
        assert call(E=0, **{name: None}) == EINVAL, name
    for name in ("store", "gather", "params", "store_t", "t_mix", "fill"):
        assert call(**{name: None}) == EINVAL, name
        assert call(B=0, **{name: None}) == EINVAL, name
        assert call(B=0, E=0, **{name: None}) == 0, name         # ... and none of them is needed without exemplars
    assert call(B=0, x_mix=None) == EINVAL and call(B=0, y_mix=None) == EINVAL
    if u8:
        assert call(lut=None) == EINVAL and call(lut=None, B=0, E=0) == 0
    assert call(B=65530, E=6) == EINVAL and call(B=0, E=65536) == EINVAL and call(B=65536, E=0) == EINVAL
    # the nothing-to-do forms
    assert call(B=0, E=0) == 0
    assert call(B=0, E=0, x=None, y=None, fill=None, lut=None, store=None, gather=None, params=None, store_t=None, x_mix=None,
                y_mix=None, t_mix=None) == 0


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
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, RandomPadCropFlip, RandomResizedCropFlip, TensorTaskDataset
    from clsurvey_amd.methods import icarl_main
    y = torch.arange(8) % 2
    x = torch.zeros((8, 3, 12, 12))
    xb = torch.zeros((8, 3, 12, 12), dtype=torch.uint8)
    mean, std = torch.full((3,), 0.5), torch.full((3,), 0.25)
    names = ["0", "1"]
    plain = TensorTaskDataset(x, y, names)
    crop = TensorTaskDataset(x, y, names, transform=RandomCropFlip((8, 8)))
    resized = TensorTaskDataset(x, y, names, transform=RandomResizedCropFlip((8, 8)))
    padded = TensorTaskDataset(x, y, names, transform=RandomPadCropFlip((12, 12), 2))
    bytes_padded = ByteTaskDataset(xb, y, names, mean, std, transform=RandomPadCropFlip((12, 12), 2, fill=(128, 3, 250)))
    bytes_crop = ByteTaskDataset(xb, y, names, mean, std, transform=RandomCropFlip((8, 8)))

    def run(train, **kw):
        return icarl_main.main(_main_args(tmp_path, train, **kw), [2, 2], device="cpu")
    for train, extra in ((plain, {}), (crop, {}), (resized, {}), (resized, dict(exemplar_resized=True)), (crop, dict(exemplar_frames=True)),
                         (bytes_crop, dict(exemplar_dtype="uint8"))):
        with pytest.raises(ValueError, match="exemplar_pad_frames=True stores the unpadded frames"):
            run(train, exemplar_pad_frames=True, **extra)
    with pytest.raises(ValueError, match="exemplar_pad_frames=True replays through a RandomPadCropFlip, exemplar_resized=True"):
        run(padded, exemplar_pad_frames=True, exemplar_resized=True)
    with pytest.raises(ValueError, match="exemplar_dtype is 'float32' or 'uint8'"):
        run(padded, exemplar_pad_frames=True, exemplar_dtype="float16")
    with pytest.raises(ValueError, match="exemplar_dtype='uint8' stores the byte frames"):
        run(padded, exemplar_pad_frames=True, exemplar_dtype="uint8")
    with pytest.raises(NotImplementedError, match="pass exemplar_dtype='uint8'"):
        run(bytes_padded, exemplar_pad_frames=True)
    with pytest.raises(ValueError, match="the fill of byte frames is ints in 0..255"):      # a byte fill per channel: the split's own rule
        ByteTaskDataset(xb, y, names, mean, std, transform=RandomPadCropFlip((12, 12), 2, fill=0.5))
    # without the switch the refusal stands, and now names it
    for extra in ({}, dict(exemplar_frames=True), dict(exemplar_pad_frames=False)):
        with pytest.raises(NotImplementedError, match="padded replay is not built.*exemplar_pad_frames=True.*--icarl_padded"):
            run(padded, **extra)
    # with it the entry gets past every check made on the split alone and as far as a CPU device goes: the prev_model_path of
    # these arguments holds an empty dict, not a wrapper, and that is what stops it
    later = os.path.join(str(tmp_path), "empty.pth.tar")
    torch.save({}, later)
    for train, extra in ((padded, {}), (padded, dict(exemplar_frames=True)), (bytes_padded, dict(exemplar_dtype="uint8"))):
        with pytest.raises(AttributeError, match="'dict' object has no attribute 'batch_size'"):
            run(train, exemplar_pad_frames=True, task_count=2, task_name="2", is_scratch_model=False, postprocess=False,
                prev_model_path=later, **extra)
    # the frame arguments a valid combination gives the wrapper
    ns = types.SimpleNamespace(exemplar_resized=False, exemplar_dtype="uint8", exemplar_pad_frames=True)
    frames = icarl_main._frame_arguments(ns, bytes_padded)
    assert frames["exemplar_transform"] is bytes_padded.transform and frames["frame_shape"] == (3, 12, 12)
    assert torch.equal(frames["frame_norm"][0], mean) and torch.equal(frames["frame_norm"][1], std)
    ns = types.SimpleNamespace(exemplar_resized=False, exemplar_dtype="float32", exemplar_pad_frames=True)
    assert set(icarl_main._frame_arguments(ns, padded)) == {"exemplar_transform", "frame_shape"}
    # a loaded wrapper's transform is of the split's class: padded, crop or resized
    specs = {"padded": padded.transform, "crop": crop.transform, "resized": resized.transform}
    for a, sa in specs.items():
        for b, sb in specs.items():
            loaded = types.SimpleNamespace(exemplar_transform=sa, frame_norm=None)
            if a == b:
                icarl_main._check_loaded(loaded, dict(exemplar_transform=sb))
            else:
                with pytest.raises(ValueError, match="the loaded wrapper replays"):
                    icarl_main._check_loaded(loaded, dict(exemplar_transform=sb))
    with pytest.raises(ValueError, match="holds crops"):
        icarl_main._check_loaded(types.SimpleNamespace(exemplar_transform=None), dict(exemplar_transform=padded.transform))
    with pytest.raises(ValueError, match="exemplar store is float32"):
        icarl_main._check_loaded(types.SimpleNamespace(exemplar_transform=padded.transform, frame_norm=None),
                                 dict(exemplar_transform=padded.transform, frame_norm=(mean, std)))


# ---------------------------------------------------------------------------------------------- method layer and driver
def test_the_method_layer_sets_the_argument_only_when_given(monkeypatch):
    """--icarl_padded reaches icarl_main.main as exemplar_pad_frames=True, exemplar_padded never does, and without the flag the
    recorded trainer arguments are what they were."""
    from clsurvey_amd.methods import method as M
    seen = []
    monkeypatch.setattr(M._icarl, "main", lambda kw, nc, device=None: seen.append(dict(kw)))

    class _Dataset:
        task_count = 2
        classes_per_task = {"1": ["a", "b"], "2": ["c", "d"]}

    def manager():
        return types.SimpleNamespace(dataset=_Dataset(), previous_task_model_path="prev", current_task_dataset_path="data",
                                     gridsearch_exp_dir="exp", overwrite_args=None)

    def args(**kw):
        return types.SimpleNamespace(task_counter=2, task_name="2", mem_per_task=4, num_epochs=1, batch_size=8, device="cpu",
                                     weight_decay=0.0, lr=0.01, **kw)
    for flags in ({}, {"icarl_padded": False}, {"icarl_padded": True}, {"icarl_padded": True, "u8_exemplars": True},
                  {"padded_exemplars": True}):
        seen.clear()
        m = manager()
        M._icarl_run(M.parse("ICARL"), args(**flags), m, 1.0, "out")
        assert len(seen) == 1 and m.overwrite_args == seen[0]
        on = bool(flags.get("icarl_padded"))
        assert ("exemplar_pad_frames" in seen[0]) == on and seen[0].get("exemplar_pad_frames", None) == (True if on else None)
        assert "exemplar_padded" not in seen[0] and "exemplar_frames" not in seen[0]
        assert seen[0].get("exemplar_dtype") == ("uint8" if flags.get("u8_exemplars") else None)


class _Reached(Exception):
    pass


def test_driver_flag_checks(tmp_path, monkeypatch):
    from clsurvey_amd.framework import driver, tasks
    argv = ["small_VGG9_cl_128_128", "--results_root", str(tmp_path), "--synthetic", "2,4,16,8,8,32", "--method_name", "ICARL"]
    for extra in ([], ["--rnd_margin", "4"], ["--rnd_resized", "4"]):
        with pytest.raises(SystemExit, match="--icarl_padded belongs with --rnd_pad"):
            driver.main(argv + ["--icarl_padded"] + extra)
    with pytest.raises(SystemExit, match="--icarl_frames belongs with"):              # (the earlier check, as before)
        driver.main(argv + ["--rnd_pad", "4", "--icarl_padded", "--icarl_frames"])
    with pytest.raises(SystemExit, match="--icarl_padded belongs with --rnd_pad"):
        driver.main(argv + ["--rnd_margin", "4", "--icarl_padded", "--icarl_frames"])
    with pytest.raises(SystemExit, match="--resized_exemplars belongs with"):
        driver.main(argv + ["--rnd_pad", "4", "--icarl_padded", "--resized_exemplars"])
    # a byte store on padded tasks needs the switch and byte frames
    with pytest.raises(SystemExit, match="--u8_exemplars belongs with"):
        driver.main(argv + ["--rnd_pad", "4", "--u8_frames", "--u8_exemplars"])
    with pytest.raises(SystemExit, match="--u8_exemplars belongs with"):
        driver.main(argv + ["--rnd_pad", "4", "--icarl_padded", "--u8_exemplars"])
    assert not os.path.exists(os.path.join(str(tmp_path), "data"))                   # raised before anything is generated
    p = driver.build_parser()
    assert p.parse_args(argv).icarl_padded is False
    assert p.parse_args(argv + ["--rnd_pad", "4", "--icarl_padded"]).icarl_padded is True

    # the valid combinations get past the argument validation: the next thing the driver does is make the task sequence
    def reached(*a, **kw):
        raise _Reached(kw)
    monkeypatch.setattr(tasks, "SyntheticTaskSequence", reached)
    for extra in (["--rnd_pad", "4", "--icarl_padded"], ["--rnd_pad", "4", "--pad_mode", "reflect", "--icarl_padded"],
                  ["--u8_frames", "--rnd_pad", "4", "--icarl_padded", "--u8_exemplars"]):
        with pytest.raises(_Reached) as info:
            driver.main(argv + extra)
        kw = info.value.args[0]
        assert kw["rnd_pad"] == 4 and kw["u8_frames"] == ("--u8_frames" in extra)


def test_the_exclusions_of_the_switch(tmp_path):
    """--icarl_padded with --icarl_frames or --resized_exemplars is a SystemExit, whichever check speaks first: on --rnd_pad tasks
    alone the two belong elsewhere, and with the augmentation they belong to the switches exclude each other."""
    from clsurvey_amd.framework import driver
    argv = ["small_VGG9_cl_128_128", "--results_root", str(tmp_path), "--synthetic", "2,4,16,8,8,32", "--method_name", "ICARL",
            "--rnd_pad", "4", "--icarl_padded"]
    for extra in (["--icarl_frames"], ["--resized_exemplars"], ["--icarl_frames", "--resized_exemplars"]):
        with pytest.raises(SystemExit):
            driver.main(argv + extra)
    with pytest.raises(SystemExit, match="--icarl_padded excludes --icarl_frames and --resized_exemplars"):
        driver.main(argv + ["--rnd_margin", "4", "--icarl_frames"])
    with pytest.raises(SystemExit, match="--icarl_padded excludes --icarl_frames and --resized_exemplars"):
        driver.main(argv + ["--rnd_resized", "4", "--resized_exemplars"])
    assert not os.path.exists(os.path.join(str(tmp_path), "data"))


# ---------------------------------------------------------------------------------------------- IcarlNet's dispatch
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_icarl_net_dispatches_the_padded_spec_to_the_padded_ops(monkeypatch, byte):
    from clsurvey_amd import ops
    from clsurvey_amd.data import RandomCropFlip, RandomPadCropFlip
    from clsurvey_amd.methods.icarl import IcarlNet
    calls = []
    names = ["icarl_assemble_pad_crop_flip", "icarl_assemble_pad_crop_flip_u8", "gather_tasks_pad_crop_flip", "gather_tasks_pad_crop_flip_u8",
             "icarl_assemble_crop_flip", "icarl_assemble_crop_flip_u8", "gather_tasks_crop_flip", "gather_tasks_crop_flip_u8",
             "icarl_assemble_resized_crop_flip", "icarl_assemble_resized_crop_flip_u8", "gather_tasks_resized_crop_flip",
             "gather_tasks_resized_crop_flip_u8"]
    for name in names:
        monkeypatch.setattr(ops, name, lambda *a, _n=name: calls.append((_n, a)) or ("crops", "labels"))

    def wrapper(spec, frame):
        w = IcarlNet.__new__(IcarlNet)
        w.device = torch.device("cpu")
        w.in_shape = (3, 12, 12)
        w._init_frames(spec, frame, (torch.full((3,), 0.5), torch.full((3,), 0.25)) if byte else None)
        w.lut, w.fill = "lut", "fill"
        w.store_x, w.store_t, w.x_mix, w.y_mix, w.t_mix = "store_x", "store_t", "x_mix", "y_mix", "t_mix"
        return w
    fill = (128, 3, 250) if byte else (0.25, -0.5, 1.0)
    w = wrapper(RandomPadCropFlip((12, 12), (1, 2, 3, 4), fill=fill, padding_mode="symmetric"), (3, 12, 12))
    assert w.params_width == 5 and w.geometry == (3, 12, 12, 12, 12) and w.store_shape == (3, 12, 12)
    assert w.store_dtype == (torch.uint8 if byte else torch.float32)
    w._assemble_step("x", "y", 7, "gather", "params")
    assert w._gather_view("table", "idx", "params") == "crops"
    w._assemble_step(None, None, 0, "gather", "params")             # the class-mean view's form
    sfx = "_u8" if byte else ""
    table = ("lut",) if byte else ()
    pad = ((3, 12, 12, 12, 12), "symmetric", (1, 2, 3, 4), "fill")
    rest = ("store_x", "gather", "params", "store_t", "x_mix", "y_mix", "t_mix")
    assert calls == [("icarl_assemble_pad_crop_flip" + sfx, pad + table + ("x", "y", 7) + rest),
                     ("gather_tasks_pad_crop_flip" + sfx, ("table",) + pad + table + ("idx", "params")),
                     ("icarl_assemble_pad_crop_flip" + sfx, pad + table + (None, None, 0) + rest)]
    # ... and the crop spec still goes where it went
    calls.clear()
    c = wrapper(RandomCropFlip((12, 12), 0.5), (3, 16, 16))
    c._assemble_step("x", "y", 7, "gather", "params")
    c._gather_view("table", "idx", "params")
    assert [n for n, _ in calls] == ["icarl_assemble_crop_flip" + sfx, "gather_tasks_crop_flip" + sfx]

