"""RandomResizedCrop + flip augmentation, the parts that need no GPU: the fp64 restatement of the filter against ATen, the
argument errors of clhip_gather_tasks_resized_crop_flip, the draws of data.draw_resized_crop_flip, the RNG contract of a loader
that carries the spec, merging and refusal, and the two task files of a sequence with `rnd_resized`."""
import math
import os
import pickle
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resized_crop_ref as ref  # noqa: E402


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- the filter
WINDOWS = [(5, 7, 8, 8), (40, 33, 8, 8), (9, 9, 4, 12), (1, 1, 8, 8), (64, 64, 56, 56), (64, 64, 8, 8)]


@pytest.mark.parametrize("h,w,th,tw", WINDOWS, ids=["%dx%d_to_%dx%d" % g for g in WINDOWS])
def test_restatement_is_atens_antialiased_bilinear_filter(h, w, th, tw):
    x = torch.randn((2, 3, h, w), generator=_gen(h * 100 + tw), dtype=torch.float64)
    want = F.interpolate(x, size=(th, tw), mode="bilinear", align_corners=False, antialias=True)
    got = ref.resize(x, th, tw)
    err = float((got - want).abs().max())
    print("restatement vs ATen float64, %dx%d -> %dx%d: %.3g" % (h, w, th, tw, err))
    assert err <= 1e-12
    for n_in, n_out in ((h, th), (w, tw)):
        W = ref.axis_weights(n_in, n_out)
        assert float((W.sum(1) - 1).abs().max()) <= 1e-15 and bool((W >= 0).all())
        assert ref.taps(n_in, n_out) <= math.ceil(2 * max(n_in / n_out, 1.0)) + 1


def test_an_identity_window_has_one_tap_of_weight_one():
    for n in (1, 7, 56):
        assert torch.equal(ref.axis_weights(n, n), torch.eye(n, dtype=torch.float64))
    assert ref.taps(64, 8) in (16, 17) and ref.taps(40, 8) <= 11


# ---------------------------------------------------------------------------------------------- the ABI
def test_argument_errors_do_not_need_a_device():
    import ctypes as C
    from clsurvey_amd import _lib
    L = _lib.lib()
    assert "clhip_gather_tasks_resized_crop_flip" in _lib.SIGNATURES
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    f = L.clhip_gather_tasks_resized_crop_flip                    # (tasks, T, C, Hs, Ws, th, tw, idx, params, B, x_out, labels_out, stream)
    assert f(None, 3, 3, 20, 20, 16, 16, one, one, 4, one, one, None) == -1
    assert f(one, 0, 3, 20, 20, 16, 16, one, one, 4, one, one, None) == -1
    assert f(one, 65, 3, 20, 20, 16, 16, one, one, 4, one, one, None) == -1
    assert f(one, 3, 3, 0, 20, 16, 16, one, one, 4, one, one, None) == -1           # Hs = 0
    assert f(one, 3, 3, 20, 0, 16, 16, one, one, 4, one, one, None) == -1           # Ws = 0
    assert f(one, 3, 3, 20, 20, 21, 16, one, one, 0, one, one, None) == 0           # th > Hs enlarges: no error
    assert f(one, 3, 3, 20, 20, 0, 16, one, one, 4, one, one, None) == -1           # th = 0
    assert f(one, 3, 3, 20, 20, 16, 0, one, one, 4, one, one, None) == -1
    assert f(one, 3, 0, 20, 20, 16, 16, one, one, 4, one, one, None) == -1          # C = 0
    assert f(one, 3, 3, 20, 20, 16, 16, None, one, 4, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, None, 4, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, 4, None, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, 4, one, None, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, 70000, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, -1, one, one, None) == -1
    assert f(one, 3, 3, 20, 20, 16, 16, one, one, 0, one, one, None) == 0           # nothing to do


def test_op_rejects_cpu_tensors_and_a_table_of_the_wrong_shape():
    from clsurvey_amd import ops
    table = torch.zeros((1, 4), dtype=torch.int64)
    idx = torch.zeros((2,), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.gather_tasks_resized_crop_flip(table, (3, 20, 20, 16, 16), idx, torch.zeros((2, 5), dtype=torch.int32))
    assert ops.RESIZE_MAX_RATIO == 8


# ---------------------------------------------------------------------------------------------- the draws
def test_spec_is_a_class_of_its_own():
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip
    s = RandomResizedCropFlip((56, 56))
    assert s.size == (56, 56) and s.scale == (0.08, 1.0) and s.ratio == (3.0 / 4.0, 4.0 / 3.0) and s.p == 0.5 and s.extents is None
    assert not isinstance(s, RandomCropFlip) and not issubclass(RandomResizedCropFlip, RandomCropFlip)
    assert not isinstance(RandomCropFlip((56, 56)), RandomResizedCropFlip)
    back = pickle.loads(pickle.dumps(RandomResizedCropFlip((8, 7), (0.2, 0.9), (0.5, 2.0), 0.25, torch.tensor([[9, 9]]))))
    assert (back.size, back.scale, back.ratio, back.p, back.extents.tolist()) == ((8, 7), (0.2, 0.9), (0.5, 2.0), 0.25, [[9, 9]])
    for bad in (dict(size=(0, 8)), dict(size=(8, 8), p=1.5), dict(size=(8, 8), scale=(0.5, 0.2)), dict(size=(8, 8), ratio=(0.0, 1.0))):
        with pytest.raises(ValueError):
            RandomResizedCropFlip(**bad)


def test_draw_is_a_function_of_the_seed_and_agrees_with_the_loop():
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    spec = RandomResizedCropFlip((16, 16))
    a = draw_resized_crop_flip(500, spec, (20, 24), _gen(11))
    b = draw_resized_crop_flip(500, spec, (20, 24), _gen(11))
    c = draw_resized_crop_flip(500, spec, (20, 24), _gen(12))
    assert a.dtype == torch.int32 and tuple(a.shape) == (500, 5) and a.is_contiguous()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.tolist() == [list(r[:5]) for r in ref.draw(500, spec, (20, 24), _gen(11))]
    assert tuple(draw_resized_crop_flip(0, spec, (20, 24), _gen(1)).shape) == (0, 5)
    # one torch.rand call of a fixed number of columns: the generator ends where n rows of 23 float64 uniforms end
    g1, g2 = _gen(11), _gen(11)
    draw_resized_crop_flip(500, spec, (20, 24), g1)
    torch.rand((500, 23), generator=g2, dtype=torch.float64)
    assert torch.equal(g1.get_state(), g2.get_state())


def test_windows_lie_inside_each_frames_own_extent():
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    n = 600
    g = _gen(3)
    ext = torch.stack([torch.randint(1, 14, (n,), generator=g), torch.randint(1, 12, (n,), generator=g)], 1)   # all inside 13 x 11
    ext[0] = torch.tensor([1, 1])
    ext[1] = torch.tensor([13, 11])
    ext[2] = torch.tensor([13, 1])
    spec = RandomResizedCropFlip((8, 7), extents=ext)
    tab = draw_resized_crop_flip(n, spec, (13, 11), _gen(5)).long()
    top, left, h, w = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3]
    assert bool((h >= 1).all()) and bool((w >= 1).all()) and bool((top >= 0).all()) and bool((left >= 0).all())
    assert bool((top + h <= ext[:, 0]).all()) and bool((left + w <= ext[:, 1]).all())
    assert tab[0, :4].tolist() == [0, 0, 1, 1]
    assert tab.tolist() == [list(r[:5]) for r in ref.draw(n, spec, (13, 11), _gen(5))]
    # in serving order: position k holds a window of the extent of sample order[k]
    order = torch.randperm(n, generator=_gen(6))
    tab = draw_resized_crop_flip(n, spec, (13, 11), _gen(5), order=order).long()
    assert bool((tab[:, 0] + tab[:, 2] <= ext[order, 0]).all()) and bool((tab[:, 1] + tab[:, 3] <= ext[order, 1]).all())
    assert tab.tolist() == [list(r[:5]) for r in ref.draw(n, spec, (13, 11), _gen(5), order=order)]
    k = int((order == 0).nonzero())
    assert tab[k, :4].tolist() == [0, 0, 1, 1]


def test_ten_failed_tries_end_in_the_central_window():
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    spec = RandomResizedCropFlip((8, 8), scale=(1, 1), ratio=(1, 1))
    tab = draw_resized_crop_flip(50, spec, (64, 8), _gen(1))                       # sqrt(64 * 8) = 22.6 > 8: no try fits
    assert all(r[:4] == [28, 0, 8, 8] for r in tab.tolist()) and set(tab[:, 4].tolist()) == {0, 1}
    assert not any(r[5] for r in ref.draw(50, spec, (64, 8), _gen(1)))
    tab = draw_resized_crop_flip(50, spec, (8, 64), _gen(1))                       # W / H above ratio[1]
    assert all(r[:4] == [0, 28, 8, 8] for r in tab.tolist())
    wide = RandomResizedCropFlip((8, 8), scale=(4, 4), ratio=(0.5, 2.0))            # four times the area never fits; inside the ratio range
    assert all(r[:4] == [0, 0, 20, 30] for r in draw_resized_crop_flip(20, wide, (20, 30), _gen(1)).tolist())


@pytest.mark.parametrize("s,side", [(0.25, 64), (0.5, 37), (0.08, 64), (1.0, 20)])
def test_fixed_scale_and_square_ratio_fix_the_side(s, side):
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    tab = draw_resized_crop_flip(200, RandomResizedCropFlip((8, 8), scale=(s, s), ratio=(1, 1)), (side, side), _gen(2)).long()
    want = int(round(math.sqrt(s) * side))
    assert bool((tab[:, 2] == want).all()) and bool((tab[:, 3] == want).all())
    assert int(tab[:, 0].max()) <= side - want and int(tab[:, 1].max()) <= side - want
    if side - want >= 4:
        assert int(tab[:, 0].max()) == side - want and int(tab[:, 0].min()) == 0    # both ends of the offset range are reached


def test_accepted_windows_keep_scale_and_ratio_up_to_the_rounding_of_the_sides():
    """An accepted try has sqrt(area aspect) within 1/2 of w and sqrt(area / aspect) within 1/2 of h, with area / (H W) in
    scale and aspect in ratio: so (w -+ 1/2)(h -+ 1/2) brackets the area and (w -+ 1/2) / (h +- 1/2) the aspect."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    H, W = 48, 64
    spec = RandomResizedCropFlip((8, 8), scale=(0.2, 0.7), ratio=(0.6, 1.9))
    tab = draw_resized_crop_flip(5000, spec, (H, W), _gen(8)).double()
    accepted = torch.tensor([r[5] for r in ref.draw(5000, spec, (H, W), _gen(8))])
    assert int(accepted.sum()) > 4500
    h, w = tab[accepted, 2], tab[accepted, 3]
    eps = 1e-9
    assert bool(((w + 0.5) * (h + 0.5) / (H * W) >= 0.2 - eps).all()) and bool(((w - 0.5) * (h - 0.5) / (H * W) <= 0.7 + eps).all())
    assert bool(((w + 0.5) / (h - 0.5) >= 0.6 - eps).all()) and bool(((w - 0.5) / (h + 0.5) <= 1.9 + eps).all())
    share = h * w / (H * W)
    assert float(share.min()) < 0.25 and float(share.max()) > 0.65                 # the range is used, not a point of it
    assert float((w / h).min()) < 0.7 and float((w / h).max()) > 1.7


def test_flip_frequency():
    """20 000 draws: the share of flips is within 4 sigma = 4 sqrt(p (1 - p) / 20000) of p."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    for p in (0.5, 0.2):
        tab = draw_resized_crop_flip(20000, RandomResizedCropFlip((16, 16), p=p), (24, 24), _gen(2024))
        share = float(tab[:, 4].double().mean())
        print("flip share at p = %s: %.4f" % (p, share))
        assert abs(share - p) <= 4 * math.sqrt(p * (1 - p) / 20000)
        assert set(tab[:, 4].tolist()) == {0, 1}
    assert int(draw_resized_crop_flip(300, RandomResizedCropFlip((16, 16), p=0.0), (24, 24), _gen(1))[:, 4].sum()) == 0
    assert int(draw_resized_crop_flip(300, RandomResizedCropFlip((16, 16), p=1.0), (24, 24), _gen(1))[:, 4].sum()) == 300


def test_draw_raises_on_extents_the_gather_cannot_serve():
    from clsurvey_amd.data import RESIZE_MAX_RATIO, RandomResizedCropFlip, draw_resized_crop_flip
    assert RESIZE_MAX_RATIO == 8
    draw_resized_crop_flip(4, RandomResizedCropFlip((8, 8)), (64, 64), _gen(1))     # exactly the limit
    with pytest.raises(ValueError):
        draw_resized_crop_flip(4, RandomResizedCropFlip((8, 8)), (65, 64), _gen(1))
    with pytest.raises(ValueError):
        draw_resized_crop_flip(4, RandomResizedCropFlip((8, 7)), (56, 57), _gen(1))
    with pytest.raises(ValueError):                                                 # an extent larger than the stored frame
        draw_resized_crop_flip(3, RandomResizedCropFlip((16, 16), extents=torch.tensor([[20, 21]] * 3)), (20, 20), _gen(1))
    with pytest.raises(ValueError):
        draw_resized_crop_flip(4, RandomResizedCropFlip((16, 16), extents=torch.tensor([[20, 20]] * 3)), (20, 20), _gen(1))


# ---------------------------------------------------------------------------------------------- RNG contract
def _pair(n=24, hw=16, m=4, **kw):
    from clsurvey_amd.data import RandomResizedCropFlip, TensorTaskDataset
    g = _gen(9)
    frames = torch.randn((n, 3, hw + m, hw + m), generator=g)
    y = torch.randint(0, 4, (n,), generator=g)
    names = [str(c) for c in range(4)]
    return (TensorTaskDataset(frames, y, names, transform=RandomResizedCropFlip((hw, hw), **kw)),
            TensorTaskDataset(frames[:, :, 2:2 + hw, 2:2 + hw], y, names))


@pytest.mark.parametrize("shuffle", [True, False])
def test_loader_with_the_spec_consumes_the_global_generator_like_a_plain_one(shuffle):
    from clsurvey_amd.data import DeviceLoader, draw_resized_crop_flip
    aug, plain = _pair()
    a, b = DeviceLoader(aug, 7, shuffle, device="cpu"), DeviceLoader(plain, 7, shuffle, device="cpu")
    assert tuple(a.x.shape) == (0, 3, 16, 16) and tuple(a.frames[0].shape) == (24, 3, 20, 20) and len(a) == len(b) == 4
    assert a.transform is aug.transform and a.geometry == (3, 20, 20, 16, 16) and b.transform is None
    torch.manual_seed(5)
    pa = a.order()
    sa = torch.get_rng_state()
    torch.manual_seed(5)
    pb = b.order()
    sb = torch.get_rng_state()
    assert torch.equal(sa, sb)
    assert (pa is None and pb is None) if not shuffle else torch.equal(pa, pb)
    t1 = a.epoch_params(pa)
    assert torch.equal(sa, torch.get_rng_state())                                   # (the table comes from a private generator)
    torch.manual_seed(5)
    base = int(torch.empty((), dtype=torch.int64).random_().item())
    assert a.base_seed == base == b.base_seed
    assert tuple(t1.shape) == (24, 5) and torch.equal(t1, draw_resized_crop_flip(24, aug.transform, (20, 20), _gen(base), order=pa))
    p2 = a.order()
    assert not torch.equal(t1, a.epoch_params(p2))


# ---------------------------------------------------------------------------------------------- dataset, merging, refusal
def test_dataset_round_trips_through_pickle_with_the_spec(tmp_path):
    from clsurvey_amd.data import RandomResizedCropFlip, TensorTaskDataset, _transform_of, load_task_datasets
    aug, plain = _pair(scale=(0.3, 0.9), p=0.25)
    back = pickle.loads(pickle.dumps(aug))
    t = back.transform
    assert isinstance(t, RandomResizedCropFlip) and (t.size, t.scale, t.ratio, t.p) == ((16, 16), (0.3, 0.9), (3.0 / 4.0, 4.0 / 3.0), 0.25)
    assert torch.equal(back.x, aug.x) and _transform_of(back) is t and _transform_of(plain) is None
    path = os.path.join(str(tmp_path), "t.pth.tar")
    torch.save({"train": aug, "val": plain, "test": plain}, path)
    got = load_task_datasets(path, "cpu")
    assert isinstance(got["train"].transform, RandomResizedCropFlip) and got["val"].transform is None
    with pytest.raises(TypeError, match="transform is None or a RandomCropFlip"):
        TensorTaskDataset(aug.x, aug.y, aug.classes, transform="flip")
    with pytest.raises(ValueError):
        TensorTaskDataset(aug.x, aug.y, aug.classes, transform=RandomResizedCropFlip((16, 16), extents=torch.full((3, 2), 18)))


def test_tasks_of_one_list_carry_specs_of_one_class_and_equal_parameters():
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip, TensorTaskDataset, merged_transform
    aug, plain = _pair()

    def with_spec(spec):
        return TensorTaskDataset(aug.x, aug.y, aug.classes, transform=spec)

    t = merged_transform([aug, aug])
    assert isinstance(t, RandomResizedCropFlip) and (t.size, t.scale, t.ratio, t.p, t.extents) == ((16, 16), (0.08, 1.0), (0.75, 4.0 / 3.0), 0.5, None)
    with pytest.raises(ValueError):
        merged_transform([aug, plain])
    with pytest.raises(ValueError):                                                 # two classes of equal size and p
        merged_transform([aug, with_spec(RandomCropFlip((16, 16)))])
    with pytest.raises(ValueError):
        merged_transform([with_spec(RandomCropFlip((16, 16))), aug])
    for other in (dict(p=0.25), dict(scale=(0.1, 1.0)), dict(ratio=(0.5, 2.0))):
        with pytest.raises(ValueError):
            merged_transform([aug, with_spec(RandomResizedCropFlip((16, 16), **other))])
    with pytest.raises(ValueError):
        merged_transform([aug, with_spec(RandomResizedCropFlip((16, 12)))])
    ext = with_spec(RandomResizedCropFlip((16, 16), extents=torch.full((24, 2), 18)))
    t = merged_transform([aug, ext])
    assert isinstance(t, RandomResizedCropFlip) and tuple(t.extents.shape) == (48, 2)
    assert t.extents[0].tolist() == [20, 20] and t.extents[24].tolist() == [18, 18]
    assert isinstance(merged_transform([with_spec(RandomCropFlip((16, 16)))] * 2), RandomCropFlip)


def test_rehearsal_entry_refuses_the_spec(tmp_path):
    """GEM and R-PM / R-FM replay stored frames with RandomCropFlip only: a train split with the resampling spec is an error,
    raised before any loader or device is touched."""
    from clsurvey_amd.methods import gem_main
    aug, plain = _pair()
    prev = os.path.join(str(tmp_path), "prev.pth.tar")
    torch.save({}, prev)
    for method in ("gem", "baseline_rehearsal_full_mem", "baseline_rehearsal_partial_mem"):
        args = dict(task_name="2", task_count=2, prev_model_path=prev, n_outputs=8, method=method, n_memories=4, n_tasks=2,
                    dataset_path={"train": aug, "val": plain, "test": plain}, postprocess=False, is_scratch_model=False)
        with pytest.raises(NotImplementedError, match="RandomResizedCropFlip"):
            gem_main.main(args, [4, 4], device="cpu")


# ---------------------------------------------------------------------------------------------- the task sequence
def _seq(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    return SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                                 name="aug2", **kw)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_rnd_resized_zero_writes_what_it_always_wrote(tmp_path):
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    with_flag, without = _seq(a, rnd_resized=0), _seq(b)
    assert with_flag.spec("1") == without.spec("1") == {"sizes": [24, 8, 8], "classes": 4, "hw": 16, "seed": 7001, "noise": 0.4,
                                                        "kind": "protos", "blobs": None}
    pa, pb = with_flag.get_task_dataset_path("1", rnd_transform=True), without.get_task_dataset_path("1", rnd_transform=True)
    assert os.path.basename(pa) == os.path.basename(pb) == "task_1.pth.tar"
    assert _bytes(pa) == _bytes(pb) and _bytes(pa[:-8] + ".spec.json") == _bytes(pb[:-8] + ".spec.json")
    assert sorted(os.listdir(os.path.dirname(pa))) == ["task_1.pth.tar", "task_1.spec.json"]
    # and with a margin of the other kind nothing changes either: the sidecar has no new key
    assert "rnd_resized" not in _seq(a, rnd_margin=4).spec("1", True)


def test_rnd_resized_writes_a_raw_and_a_resampled_file_of_the_same_images(tmp_path):
    from clsurvey_amd.data import RandomResizedCropFlip
    ds = _seq(str(tmp_path), rnd_resized=4)
    raw_path = ds.get_task_dataset_path("2")
    aug_path = ds.get_task_dataset_path("2", rnd_transform=True)
    assert os.path.basename(raw_path) == "task_2.pth.tar" and os.path.basename(aug_path) == "task_2_rndtrans.pth.tar"
    assert ds.spec("2") == {"sizes": [24, 8, 8], "classes": 4, "hw": 16, "seed": 7002, "noise": 0.4, "kind": "protos", "blobs": None,
                            "rnd_resized": 4}
    assert ds.spec("2", True)["rnd_transform"] is True and "rnd_margin" not in ds.spec("2", True) and ds.input_size == (16, 16)
    raw, aug = torch.load(raw_path, weights_only=False), torch.load(aug_path, weights_only=False)
    t = aug["train"].transform
    assert isinstance(t, RandomResizedCropFlip) and (t.size, t.scale, t.ratio, t.p, t.extents) == ((16, 16), (0.08, 1.0), (0.75, 4.0 / 3.0), 0.5, None)
    assert tuple(aug["train"].x.shape) == (24, 3, 20, 20) and tuple(raw["train"].x.shape) == (24, 3, 16, 16)
    assert torch.equal(raw["train"].x, aug["train"].x[:, :, 2:18, 2:18]) and torch.equal(raw["train"].y, aug["train"].y)
    for split in ("val", "test"):
        assert torch.equal(raw[split].x, aug[split].x) and torch.equal(raw[split].y, aug[split].y)
        assert aug[split].transform is None and raw[split].transform is None and tuple(raw[split].x.shape) == (8, 3, 16, 16)
    assert raw["train"].transform is None
    assert sorted(os.listdir(os.path.dirname(raw_path))) == ["task_2.pth.tar", "task_2.spec.json", "task_2_rndtrans.pth.tar",
                                                             "task_2_rndtrans.spec.json"]
    # which file a method gets: the rule of rnd_margin
    always = _seq(str(tmp_path), rnd_resized=4, rnd_always=True)
    assert always.get_task_dataset_path("2", rnd_transform=False) == aug_path == always.get_task_dataset_path("2", True)
    # the same images under the other transform, or another margin, are another spec: an error, not a hit
    with pytest.raises(RuntimeError):
        _seq(str(tmp_path), rnd_margin=4).get_task_dataset_path("2", True)
    with pytest.raises(RuntimeError):
        _seq(str(tmp_path), rnd_resized=6).get_task_dataset_path("2")
    with pytest.raises(ValueError):
        _seq(str(tmp_path), rnd_resized=4, rnd_margin=4)
    with pytest.raises(ValueError):
        _seq(str(tmp_path), rnd_resized=-1)


def test_driver_flag_excludes_the_margin_and_needs_the_synthetic_sequence(tmp_path):
    from clsurvey_amd.framework import driver
    common = ["small_VGG9_cl_128_128", "--method_name", "EWC", "--results_root", str(tmp_path)]
    with pytest.raises(SystemExit):
        driver.main(common + ["--rnd_resized", "4"])
    with pytest.raises(SystemExit):
        driver.main(common + ["--synthetic", "2,4,160,40,40,32", "--rnd_resized", "4", "--rnd_margin", "4"])
    assert not os.path.exists(os.path.join(str(tmp_path), "data"))
    assert driver.build_parser().parse_args(common).rnd_resized == 0
