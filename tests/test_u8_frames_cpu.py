"""Byte frames, the parts that need no GPU: the three ..._u8 entries are exported and check their arguments, ByteTaskDataset
validates, decodes bitwise as ToTensor -> Normalize and pickles with its class, tasks served as one agree on how their frames are
stored, and the task files of a sequence with u8_frames."""
import io
import json
import os
import pickle

import pytest
import torch

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
AWKWARD = ((0.1, 1.0 / 3.0, 0.9), (1.0 / 3.0, 0.07, 3.0))


def test_entries_are_exported_and_declared():
    from clsurvey_amd import _lib, ops
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clhip.h")).read()
    for name in ("clhip_gather_tasks_u8", "clhip_gather_tasks_crop_flip_u8", "clhip_gather_tasks_resized_crop_flip_u8"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and ("int %s(const clhip_task_src_u8* tasks_dev" % name) in header
        assert callable(getattr(ops, name[len("clhip_"):]))
    assert "typedef struct clhip_task_src_u8 { const uint8_t* x; const int64_t* labels; int64_t cum_rows; int64_t label_shift; }" in header


def test_argument_errors_do_not_need_a_device():
    import ctypes as C
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = L.clhip_gather_tasks_u8                                   # (tasks, T, C, plane_elems, lut, idx, B, x_out, labels_out, stream)
    assert f(None, 3, 3, 64, one, one, 4, one, one, None) == -1
    assert f(one, 0, 3, 64, one, one, 4, one, one, None) == -1
    assert f(one, 65, 3, 64, one, one, 4, one, one, None) == -1
    assert f(one, 3, 0, 64, one, one, 4, one, one, None) == -1                      # C < 1
    assert f(one, 3, -1, 64, one, one, 4, one, one, None) == -1
    assert f(one, 3, 3, 0, one, one, 4, one, one, None) == -1                       # plane_elems < 1
    assert f(one, 3, 3, 64, None, one, 4, one, one, None) == -1                     # lut == NULL
    assert f(one, 3, 3, 64, None, one, 0, one, one, None) == -1                     # ... also with nothing to do
    assert f(one, 3, 3, 64, one, None, 4, one, one, None) == -1
    assert f(one, 3, 3, 64, one, one, 4, None, one, None) == -1
    assert f(one, 3, 3, 64, one, one, 4, one, None, None) == -1
    assert f(one, 3, 3, 64, one, one, 70000, one, one, None) == -1
    assert f(one, 3, 3, 64, one, one, -1, one, one, None) == -1
    assert f(one, 3, 3, 64, one, one, 0, one, one, None) == 0                       # nothing to do
    f = L.clhip_gather_tasks_crop_flip_u8                         # (tasks, T, C, Hs, Ws, th, tw, lut, idx, params, B, x_out, labels_out, stream)
    ok = dict(tasks=one, T=3, C=3, Hs=20, Ws=20, th=16, tw=16, lut=one, idx=one, params=one, B=4, x_out=one, labels_out=one, stream=None)

    def call(fn, **kw):
        return fn(*{**ok, **kw}.values())
    for bad in (dict(tasks=None), dict(T=0), dict(T=65), dict(th=21), dict(tw=21), dict(th=0), dict(tw=0), dict(C=0), dict(lut=None),
                dict(lut=None, B=0), dict(idx=None), dict(params=None), dict(x_out=None), dict(labels_out=None), dict(B=70000), dict(B=-1)):
        assert call(f, **bad) == -1, bad
    assert call(f, B=0) == 0
    f = L.clhip_gather_tasks_resized_crop_flip_u8                 # the same arguments; th > Hs is an enlargement, not an error
    for bad in (dict(tasks=None), dict(T=0), dict(T=65), dict(Hs=0), dict(Ws=0), dict(th=0), dict(tw=0), dict(th=-1), dict(C=0),
                dict(lut=None), dict(lut=None, B=0), dict(idx=None), dict(params=None), dict(x_out=None), dict(labels_out=None),
                dict(B=70000), dict(B=-1)):
        assert call(f, **bad) == -1, bad
    assert call(f, B=0) == 0 and call(f, B=0, th=21, tw=40) == 0
    # CLHIP_ENOTSUP from the plan as for the fp32 entry, before any launch
    g = L.clhip_gather_tasks_resized_crop_flip
    fp32 = {k: v for k, v in ok.items() if k != "lut"}
    assert g(*{**fp32, "Hs": 1000, "Ws": 1000, "th": 125, "tw": 125}.values()) == -3
    assert call(f, Hs=1000, Ws=1000, th=125, tw=125) == -3


def _frames(n=4, C=3, H=16, W=16):
    """Frames that contain all 256 values in every channel."""
    assert H * W == 256
    x = torch.stack([torch.arange(256, dtype=torch.uint8)[torch.randperm(256, generator=torch.Generator().manual_seed(k))]
                     for k in range(n * C)]).view(n, C, H, W)
    assert all(len(set(x[0, c].reshape(-1).tolist())) == 256 for c in range(C))
    return x


def test_validation():
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, TensorTaskDataset
    x, y = _frames(), torch.tensor([0, 1, 2, 3])
    mean, std = IMAGENET
    d = ByteTaskDataset(x, y, list("abcd"), mean, std)
    assert isinstance(d, TensorTaskDataset) and d.x.dtype == torch.uint8 and d.x.element_size() == 1 and len(d) == 4
    assert d.mean.dtype == torch.float32 and d.std.dtype == torch.float32 and not d.mean.is_cuda and d.transform is None
    assert d[1][0].dtype == torch.uint8 and int(d[1][1]) == 1
    with pytest.raises(TypeError):
        ByteTaskDataset(x.float(), y, [], mean, std)
    with pytest.raises(TypeError):
        ByteTaskDataset(x.to(torch.int8), y, [], mean, std)
    with pytest.raises(ValueError):
        ByteTaskDataset(x.view(4, 3, 256), y, [], mean, std)
    with pytest.raises(ValueError):
        ByteTaskDataset(x, y, [], mean[:2], std)
    with pytest.raises(ValueError):
        ByteTaskDataset(x, y, [], mean, std + (1.0,))
    for bad in ((0.2, 0.0, 0.2), (0.2, -0.1, 0.2), (0.2, float("inf"), 0.2), (0.2, float("nan"), 0.2)):
        with pytest.raises(ValueError):
            ByteTaskDataset(x, y, [], mean, bad)
    with pytest.raises(ValueError):
        ByteTaskDataset(x, y, [], (0.1, float("nan"), 0.1), std)
    with pytest.raises(TypeError):
        ByteTaskDataset(x, y, [], mean, std, transform="flip")
    with pytest.raises(ValueError):
        ByteTaskDataset(x, y, [], mean, std, transform=RandomCropFlip((8, 8), extents=torch.full((3, 2), 16)))
    assert ByteTaskDataset(x, y, [], mean, std, transform=RandomCropFlip((8, 8))).transform.size == (8, 8)
    # TensorTaskDataset itself: a uint8 tensor still becomes floats 0..255
    t = TensorTaskDataset(x, y, [])
    assert t.x.dtype == torch.float32 and float(t.x.max()) == 255.0


@pytest.mark.parametrize("mean,std", [IMAGENET, AWKWARD], ids=["imagenet", "awkward"])
def test_decoded_is_to_tensor_then_normalize_bitwise(mean, std):
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, TensorTaskDataset
    x, y = _frames(), torch.tensor([3, 1, 0, 2])
    spec = RandomCropFlip((8, 8))
    d = ByteTaskDataset(x, y, list("abcd"), mean, std, transform=spec)
    m, s = torch.tensor(mean), torch.tensor(std)
    want = (x.float().div(255) - m[:, None, None]) / s[:, None, None]
    dec = d.decoded()
    assert type(dec) is TensorTaskDataset and dec.x.dtype == torch.float32
    assert torch.equal(dec.x.view(torch.int32), want.view(torch.int32))
    assert torch.equal(dec.y, d.y) and dec.classes == d.classes and dec.transform is spec
    lut = d.lut()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and not lut.is_cuda
    assert torch.equal(lut, (torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)[None, :] - m[:, None]) / s[:, None])
    assert d.x.dtype == torch.uint8                               # decoding leaves the dataset as it was


def test_pickle_round_trip_and_a_dict_passes_through():
    from clsurvey_amd.data import ByteTaskDataset, RandomResizedCropFlip, load_task_datasets
    x, y = _frames(), torch.tensor([0, 1, 2, 3])
    d = ByteTaskDataset(x, y, list("abcd"), *AWKWARD, transform=RandomResizedCropFlip((8, 8)))
    for back in (pickle.loads(pickle.dumps(d)), _torch_roundtrip(d)):
        assert type(back) is ByteTaskDataset and back.x.dtype == torch.uint8 and torch.equal(back.x, d.x) and torch.equal(back.y, d.y)
        assert torch.equal(back.mean, d.mean) and torch.equal(back.std, d.std) and back.classes == d.classes
        assert isinstance(back.transform, RandomResizedCropFlip) and torch.equal(back.lut(), d.lut())
    dsets = {"train": d, "val": d, "test": d}
    assert load_task_datasets(dsets) is dsets


def _torch_roundtrip(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def test_tasks_served_as_one_agree_on_their_frames():
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, TaskList, merged_norm, merged_transform
    from clsurvey_amd.methods.method import ConcatTasks
    x, y = _frames(), torch.tensor([0, 1, 0, 1])
    spec = RandomCropFlip((8, 8))
    a = ByteTaskDataset(x, y, ["a", "b"], *IMAGENET, transform=spec)
    b = ByteTaskDataset(x.flip(0), y, ["c", "d"], *IMAGENET, transform=spec)
    other = ByteTaskDataset(x, y, ["c", "d"], IMAGENET[0], (0.229, 0.224, 0.226), transform=spec)
    other_mean = ByteTaskDataset(x, y, ["c", "d"], (0.485, 0.456, 0.407), IMAGENET[1], transform=spec)
    fl = a.decoded()
    assert merged_norm([fl, fl]) is None and merged_transform([fl, fl]).size == (8, 8)
    mean, std = merged_norm([a, b])
    assert torch.equal(mean, a.mean) and torch.equal(std, a.std) and merged_transform([a, b]).size == (8, 8)
    for fn in (merged_norm, merged_transform, TaskList, lambda ds: ConcatTasks(ds, [2, 2])):
        for mixed in ([a, fl], [fl, a], [a, other], [a, other_mean], [a, b, other]):
            with pytest.raises(ValueError):
                fn(mixed)
    tl = TaskList([a, b])
    assert len(tl) == 8 and tl[5][0].dtype == torch.uint8 and int(tl[5][1]) == int(b.y[1]) + 2
    assert tl.datasets[0].x.data_ptr() == a.x.data_ptr()         # references, no merged copy
    c = ConcatTasks([a, b], [2, 2])
    assert type(c) is ByteTaskDataset and c.x.dtype == torch.uint8 and tuple(c.x.shape) == (8, 3, 16, 16)
    assert torch.equal(c.x, torch.cat([a.x, b.x])) and c.y.tolist() == [0, 1, 0, 1, 2, 3, 2, 3] and c.classes == list("abcd")
    assert torch.equal(c.mean, a.mean) and torch.equal(c.std, a.std) and c.transform.size == (8, 8)
    f = ConcatTasks([fl, b.decoded()], [2, 2])
    assert type(f) is ConcatTasks and f.x.dtype == torch.float32 and torch.equal(f.x, c.decoded().x) and torch.equal(f.y, c.y)


def test_rehearsal_entry_refuses_an_augmented_byte_split(tmp_path):
    """Frame-mode exemplar stores are fp32: raised before any loader or device is touched."""
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip
    from clsurvey_amd.methods import gem_main
    x, y = _frames(), torch.tensor([0, 1, 2, 3])
    aug = ByteTaskDataset(x, y, list("abcd"), *IMAGENET, transform=RandomCropFlip((8, 8)))
    plain = ByteTaskDataset(x[:, :, :8, :8], y, list("abcd"), *IMAGENET)
    prev = os.path.join(str(tmp_path), "prev.pth.tar")
    torch.save({}, prev)
    for method in ("gem", "baseline_rehearsal_full_mem", "baseline_rehearsal_partial_mem"):
        args = dict(task_name="2", task_count=2, prev_model_path=prev, n_outputs=8, method=method, n_memories=4, n_tasks=2,
                    dataset_path={"train": aug, "val": plain, "test": plain}, postprocess=False, is_scratch_model=False)
        with pytest.raises(NotImplementedError, match="byte frames"):
            gem_main.main(args, [4, 4], device="cpu")


# ---------------------------------------------------------------------------------------------- the task sequence
def _seq(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    return SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                                 name="seq", **kw)


def _spec(path):
    with open(path.replace(".pth.tar", ".spec.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("margin", [{}, {"rnd_margin": 4}, {"rnd_resized": 4}], ids=["plain", "rnd_margin", "rnd_resized"])
def test_sequence_with_u8_frames_writes_the_quantised_images(tmp_path, margin):
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip, RandomResizedCropFlip, TensorTaskDataset
    fl, by = _seq(os.path.join(str(tmp_path), "f"), **margin), _seq(os.path.join(str(tmp_path), "b"), u8_frames=True, **margin)
    for rnd in ([False, True] if margin else [False]):
        pf, pb = fl.get_task_dataset_path("1", rnd), by.get_task_dataset_path("1", rnd)
        assert os.path.basename(pf) == os.path.basename(pb) == ("task_1_rndtrans.pth.tar" if rnd else "task_1.pth.tar")
        sf, sb = _spec(pf), _spec(pb)
        assert "u8_frames" not in sf and sb == {**sf, "u8_frames": True}
        df, db = torch.load(pf, weights_only=False), torch.load(pb, weights_only=False)
        for split in ("train", "val", "test"):
            f, b = df[split], db[split]
            assert type(f) is TensorTaskDataset and type(b) is ByteTaskDataset and b.x.dtype == torch.uint8
            assert torch.equal(b.x, (f.x * 48 + 128).round().clamp(0, 255).to(torch.uint8)) and torch.equal(b.y, f.y) and b.classes == f.classes
            assert torch.equal(b.mean, torch.full((3,), 128.0 / 255)) and torch.equal(b.std, torch.full((3,), 48.0 / 255))
            assert type(b.transform) is type(f.transform)
            inside = ((f.x * 48 + 128) >= 0) & ((f.x * 48 + 128) <= 255)          # where nothing was clamped: half a grey level
            assert bool(inside.any()) and float((b.decoded().x - f.x)[inside].abs().max()) <= 0.5 / 48 + 1e-5
        want = {"rnd_margin": RandomCropFlip, "rnd_resized": RandomResizedCropFlip}.get(next(iter(margin), None)) if rnd else None
        assert (db["train"].transform is None) if want is None else isinstance(db["train"].transform, want)
        assert tuple(db["train"].x.shape[1:]) == ((3, 20, 20) if rnd else (3, 16, 16)) and tuple(db["test"].x.shape[1:]) == (3, 16, 16)
        assert os.path.getsize(pb) < os.path.getsize(pf)


def test_a_cached_float_file_of_the_same_root_is_an_error_not_a_hit(tmp_path):
    root = str(tmp_path)
    _seq(root).get_task_dataset_path("1")
    with pytest.raises(RuntimeError, match="was generated from"):
        _seq(root, u8_frames=True).get_task_dataset_path("1")
    other = os.path.join(root, "other")
    _seq(other, u8_frames=True).get_task_dataset_path("1")
    with pytest.raises(RuntimeError, match="was generated from"):
        _seq(other).get_task_dataset_path("1")


def test_without_the_option_the_spec_keys_are_todays(tmp_path):
    s = _seq(str(tmp_path))
    assert sorted(s.spec("1")) == ["blobs", "classes", "hw", "kind", "noise", "seed", "sizes"]
    assert sorted(_seq(str(tmp_path), rnd_margin=4).spec("1", True)) == ["blobs", "classes", "hw", "kind", "noise", "rnd_margin",
                                                                         "rnd_transform", "seed", "sizes"]
    assert sorted(_seq(str(tmp_path), u8_frames=True).spec("1")) == ["blobs", "classes", "hw", "kind", "noise", "seed", "sizes", "u8_frames"]
    a = _seq(os.path.join(str(tmp_path), "a")).get_task_dataset_path("2")
    b = _seq(os.path.join(str(tmp_path), "b"), u8_frames=False).get_task_dataset_path("2")
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    assert _spec(a) == _spec(b)


def test_u8_frames_belongs_to_synthetic(tmp_path):
    from clsurvey_amd.framework import driver
    with pytest.raises(SystemExit, match="--u8_frames belongs to --synthetic"):
        driver.main(["small_VGG9_cl_128_128", "--results_root", str(tmp_path), "--method_name", "EWC", "--u8_frames"])
