"""On-device crop + flip augmentation, the parts that need no GPU: argument errors of clhip_gather_tasks_crop_flip, the
draws of data.draw_crop_flip, the RNG contract of an augmented loader and the two task files of a sequence with a margin."""
import os
import pickle

import pytest
import torch


def test_argument_errors_do_not_need_a_device():
    import ctypes as C
    from clsurvey_amd import _lib
    L = _lib.lib()
    assert "clhip_gather_tasks_crop_flip" in _lib.SIGNATURES
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = L.clhip_gather_tasks_crop_flip                            # (tasks, T, C, Hs, Ws, th, tw, idx, params, B, x_out, labels_out, stream)
    assert f(None, 3, 3, 20, 20, 16, 16, one, one, 4, one, one, None) == -1
    assert f(one, 0, 3, 20, 20, 16, 16, one, one, 4, one, one, None) == -1
    assert f(one, 65, 3, 20, 20, 16, 16, one, one, 4, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 21, 16, one, one, 4, one, one, None) == -1          # th > Hs
    assert f(one, 3, 3, 20, 20, 16, 21, one, one, 4, one, one, None) == -1          # tw > Ws
    assert f(one, 3, 3, 20, 20, 0, 16, one, one, 4, one, one, None) == -1           # th = 0
    assert f(one, 3, 3, 20, 20, 16, 0, one, one, 4, one, one, None) == -1
    assert f(one, 3, 0, 20, 20, 16, 16, one, one, 4, one, one, None) == -1          # C = 0
    assert f(one, 3, 3, 20, 20, 16, 16, None, one, 4, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, None, 4, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, 70000, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, -1, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, 0, one, one, None) == 0           # nothing to do


# ---------------------------------------------------------------------------------------------- draw_crop_flip
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_draw_is_a_function_of_the_seed():
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    spec = RandomCropFlip((16, 16))
    a = draw_crop_flip(500, spec, (20, 24), _gen(11))
    b = draw_crop_flip(500, spec, (20, 24), _gen(11))
    c = draw_crop_flip(500, spec, (20, 24), _gen(12))
    assert a.dtype == torch.int32 and tuple(a.shape) == (500, 3) and a.is_contiguous()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(a[:, 0].min()) >= 0 and int(a[:, 0].max()) <= 4 and int(a[:, 1].min()) >= 0 and int(a[:, 1].max()) <= 8
    assert tuple(draw_crop_flip(0, spec, (20, 24), _gen(1)).shape) == (0, 3)


def test_draw_stays_inside_each_frames_own_extent():
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    n = 600
    g = _gen(3)
    ext = torch.stack([torch.randint(8, 14, (n,), generator=g), torch.randint(7, 12, (n,), generator=g)], 1)   # all below 13 x 11
    ext[0] = torch.tensor([8, 7])                                                  # size == extent: no freedom
    ext[1] = torch.tensor([13, 11])
    spec = RandomCropFlip((8, 7), extents=ext)
    tab = draw_crop_flip(n, spec, (13, 11), _gen(5)).long()
    assert bool((tab[:, 0] >= 0).all()) and bool((tab[:, 0] <= ext[:, 0] - 8).all())
    assert bool((tab[:, 1] >= 0).all()) and bool((tab[:, 1] <= ext[:, 1] - 7).all())
    assert tab[0, 0] == 0 and tab[0, 1] == 0
    assert int((tab[:, 0] == ext[:, 0] - 8).sum()) > 0 and int((tab[:, 1] == ext[:, 1] - 7).sum()) > 0   # the upper end is reached
    # in serving order: position k holds the extent of sample order[k]
    order = torch.randperm(n, generator=_gen(6))
    tab = draw_crop_flip(n, spec, (13, 11), _gen(5), order=order).long()
    assert bool((tab[:, 0] <= ext[order, 0] - 8).all()) and bool((tab[:, 1] <= ext[order, 1] - 7).all())
    k = int((order == 0).nonzero())
    assert tab[k, 0] == 0 and tab[k, 1] == 0


def test_draw_without_freedom_and_flip_probabilities():
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    tab = draw_crop_flip(300, RandomCropFlip((16, 16), p=0.0), (16, 16), _gen(1))
    assert int(tab.abs().sum()) == 0
    tab = draw_crop_flip(300, RandomCropFlip((16, 16), p=1.0), (16, 16), _gen(1))
    assert int(tab[:, :2].abs().sum()) == 0 and bool((tab[:, 2] == 1).all())


def test_draw_raises_on_an_extent_below_the_crop():
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    with pytest.raises(ValueError):
        draw_crop_flip(4, RandomCropFlip((16, 16)), (16, 15), _gen(1))
    ext = torch.tensor([[20, 20], [15, 20], [20, 20]])
    with pytest.raises(ValueError):
        draw_crop_flip(3, RandomCropFlip((16, 16), extents=ext), (20, 20), _gen(1))
    with pytest.raises(ValueError):                                                 # an extent larger than the stored frame
        draw_crop_flip(3, RandomCropFlip((16, 16), extents=torch.tensor([[20, 21]] * 3)), (20, 20), _gen(1))
    with pytest.raises(ValueError):
        RandomCropFlip((0, 16))


def test_draw_distribution():
    """20 000 draws, 9 possible offsets: every value occurs (a value missing from 20 000 uniform draws has probability
    9 (8/9)^20000 ~ 0) and each share is within 1/9 +- 0.01 (4.5 sigma of sqrt(1/9 * 8/9 / 20000) = 0.0022); the flip share is
    within 0.5 +- 0.02 (5.6 sigma of 0.0035)."""
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    tab = draw_crop_flip(20000, RandomCropFlip((16, 16)), (24, 24), _gen(2024)).long()
    for col in (0, 1):
        counts = torch.bincount(tab[:, col], minlength=9)
        print("offset counts, column", col, counts.tolist())
        assert counts.numel() == 9 and int(counts.min()) > 0
        assert float((counts.double() / 20000 - 1.0 / 9).abs().max()) < 0.01
    share = float(tab[:, 2].double().mean())
    print("flip share", share)
    assert abs(share - 0.5) <= 0.02
    assert set(tab[:, 2].tolist()) == {0, 1}


# ---------------------------------------------------------------------------------------------- RNG contract
def _pair(n=24, hw=16, m=4):
    from clsurvey_amd.data import RandomCropFlip, TensorTaskDataset
    g = _gen(9)
    frames = torch.randn((n, 3, hw + m, hw + m), generator=g)
    y = torch.randint(0, 4, (n,), generator=g)
    names = [str(c) for c in range(4)]
    return (TensorTaskDataset(frames, y, names, transform=RandomCropFlip((hw, hw))),
            TensorTaskDataset(frames[:, :, 2:2 + hw, 2:2 + hw], y, names))


@pytest.mark.parametrize("shuffle", [True, False])
def test_augmented_loader_consumes_the_global_generator_like_a_plain_one(shuffle):
    from clsurvey_amd.data import DeviceLoader
    aug, plain = _pair()
    a, b = DeviceLoader(aug, 7, shuffle, device="cpu"), DeviceLoader(plain, 7, shuffle, device="cpu")
    assert tuple(a.x.shape) == (0, 3, 16, 16) and tuple(a.frames[0].shape) == (24, 3, 20, 20) and len(a) == len(b) == 4
    assert b.transform is None and tuple(b.x.shape) == (24, 3, 16, 16)
    torch.manual_seed(5)
    pa = a.order()
    sa = torch.get_rng_state()
    torch.manual_seed(5)
    pb = b.order()
    sb = torch.get_rng_state()
    assert torch.equal(sa, sb)
    assert (pa is None and pb is None) if not shuffle else torch.equal(pa, pb)
    # the private generator is seeded with the base seed order() drew first
    torch.manual_seed(5)
    base = int(torch.empty((), dtype=torch.int64).random_().item())
    assert a.base_seed == base == b.base_seed


def test_two_epochs_draw_different_tables():
    from clsurvey_amd.data import DeviceLoader, draw_crop_flip
    aug, _ = _pair()
    loader = DeviceLoader(aug, 7, True, device="cpu")
    torch.manual_seed(5)
    p1 = loader.order()
    t1 = loader.epoch_params(p1)
    assert torch.equal(t1, draw_crop_flip(24, aug.transform, (20, 20), _gen(loader.base_seed), order=p1))
    p2 = loader.order()
    t2 = loader.epoch_params(p2)
    assert tuple(t1.shape) == tuple(t2.shape) == (24, 3) and not torch.equal(t1, t2)
    assert int(t1[:, :2].max()) <= 4 and int(t1.min()) >= 0


def test_tasks_of_one_list_carry_equal_transforms_or_none():
    from clsurvey_amd.data import RandomCropFlip, TensorTaskDataset, merged_transform
    aug, plain = _pair()
    other = TensorTaskDataset(aug.x, aug.y, aug.classes, transform=RandomCropFlip((16, 16), p=0.25))
    assert merged_transform([plain, plain]) is None
    t = merged_transform([aug, aug])
    assert t.size == (16, 16) and t.p == 0.5 and t.extents is None
    with pytest.raises(ValueError):
        merged_transform([aug, plain])
    with pytest.raises(ValueError):
        merged_transform([aug, other])
    ext = TensorTaskDataset(aug.x, aug.y, aug.classes, transform=RandomCropFlip((16, 16), extents=torch.full((24, 2), 18)))
    t = merged_transform([aug, ext])
    assert tuple(t.extents.shape) == (48, 2) and t.extents[0].tolist() == [20, 20] and t.extents[24].tolist() == [18, 18]
    x0, y0 = aug[3]                                               # __getitem__ stays the stored frame
    assert tuple(x0.shape) == (3, 20, 20)


# ---------------------------------------------------------------------------------------------- the task sequence
def _seq(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    return SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                                 name="aug2", **kw)


def test_no_margin_writes_what_it_always_wrote(tmp_path):
    from clsurvey_amd.data import synthetic_task
    ds = _seq(str(tmp_path))
    assert ds.spec("1") == {"sizes": [24, 8, 8], "classes": 4, "hw": 16, "seed": 7001, "noise": 0.4, "kind": "protos", "blobs": None}
    path = ds.get_task_dataset_path("1")
    assert path == ds.get_task_dataset_path("1", rnd_transform=True) == os.path.join(str(tmp_path), "data", "aug2", "task_1.pth.tar")
    assert _seq(str(tmp_path), rnd_always=True).get_task_dataset_path("1") == path
    assert sorted(os.listdir(os.path.dirname(path))) == ["task_1.pth.tar", "task_1.spec.json"]
    got = torch.load(path, weights_only=False)
    want = synthetic_task(24, 8, 8, 4, 16, seed=7001, noise=0.4)
    for split in ("train", "val", "test"):
        assert torch.equal(got[split].x, want[split].x) and torch.equal(got[split].y, want[split].y)
        assert got[split].transform is None and "transform" not in got[split].__dict__
    assert ds.get_task_dataset_path(None) is None and ds.input_size == (16, 16)


def test_margin_writes_a_raw_and_an_augmented_file_of_the_same_images(tmp_path):
    from clsurvey_amd.data import RandomCropFlip
    ds = _seq(str(tmp_path), rnd_margin=4)
    raw_path = ds.get_task_dataset_path("2")
    aug_path = ds.get_task_dataset_path("2", rnd_transform=True)
    assert os.path.basename(raw_path) == "task_2.pth.tar" and os.path.basename(aug_path) == "task_2_rndtrans.pth.tar"
    assert ds.spec("2")["rnd_margin"] == 4 and ds.input_size == (16, 16) and ds.get_task_dataset_path(None, True) is None
    raw, aug = torch.load(raw_path, weights_only=False), torch.load(aug_path, weights_only=False)
    t = aug["train"].transform
    assert isinstance(t, RandomCropFlip) and t.size == (16, 16) and t.p == 0.5 and t.extents is None
    assert tuple(aug["train"].x.shape) == (24, 3, 20, 20) and tuple(raw["train"].x.shape) == (24, 3, 16, 16)
    assert torch.equal(raw["train"].x, aug["train"].x[:, :, 2:18, 2:18]) and torch.equal(raw["train"].y, aug["train"].y)
    for split in ("val", "test"):
        assert torch.equal(raw[split].x, aug[split].x) and torch.equal(raw[split].y, aug[split].y)
        assert aug[split].transform is None and raw[split].transform is None and tuple(raw[split].x.shape) == (8, 3, 16, 16)
    assert raw["train"].transform is None
    # a second call is a cache hit: the files are not rewritten
    stamps = {p: os.stat(p).st_mtime_ns for p in (raw_path, aug_path)}
    assert ds.get_task_dataset_path("2") == raw_path and ds.get_task_dataset_path("2", True) == aug_path
    assert stamps == {p: os.stat(p).st_mtime_ns for p in (raw_path, aug_path)}
    assert sorted(os.listdir(os.path.dirname(raw_path))) == ["task_2.pth.tar", "task_2.spec.json", "task_2_rndtrans.pth.tar",
                                                             "task_2_rndtrans.spec.json"]
    # the RecogSeq rule: the argument is ignored
    always = _seq(str(tmp_path), rnd_margin=4, rnd_always=True)
    assert always.get_task_dataset_path("2", rnd_transform=False) == aug_path == always.get_task_dataset_path("2", True)
    assert always.get_task_dataset_path(None) is None
    # another margin under the same root is another spec: an error, not a hit
    with pytest.raises(RuntimeError):
        _seq(str(tmp_path), rnd_margin=6).get_task_dataset_path("2")


def test_a_task_file_pickled_without_the_attribute_loads(tmp_path):
    from clsurvey_amd.data import TensorTaskDataset, load_task_datasets
    d = TensorTaskDataset(torch.zeros(3, 3, 4, 4), torch.zeros(3, dtype=torch.int64), ["a"])
    assert "transform" not in d.__dict__                          # what a file written before the attribute existed holds
    back = pickle.loads(pickle.dumps({"train": d}))
    assert back["train"].transform is None
    path = os.path.join(str(tmp_path), "old.pth.tar")
    torch.save({"train": d, "val": d, "test": d}, path)
    assert all(v.transform is None for v in load_task_datasets(path, "cpu").values())
