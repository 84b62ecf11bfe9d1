"""Padded RandomCrop + flip augmentation, the parts that need no GPU: the index-map restatement (tests/pad_crop_ref.py) against
torch.nn.functional.pad, the RandomPadCropFlip spec, the draws of data.draw_pad_crop_flip, merging and the fill of decoded byte
splits, the argument errors of clhip_gather_tasks_pad_crop_flip[_u8], the refusal by the methods that replay exemplars, and the
task files of a sequence with `rnd_pad`."""
import os
import pickle
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pad_crop_ref as ref  # noqa: E402


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- the restatement
def test_the_documented_one_dimensional_examples():
    x = torch.tensor([1.0, 2.0, 3.0, 4.0])
    for mode, want in (("reflect", [3, 2, 1, 2, 3, 4, 3, 2]), ("symmetric", [2, 1, 1, 2, 3, 4, 4, 3]),
                       ("edge", [1, 1, 1, 2, 3, 4, 4, 4]), ("constant", [9, 9, 1, 2, 3, 4, 9, 9])):
        got = [9.0 if ref.pad_map(s, 4, mode) is None else float(x[ref.pad_map(s, 4, mode)]) for s in range(-2, 6)]
        assert got == [float(v) for v in want], mode
        frame = x.view(1, 1, 4)
        assert ref.window(frame, 0, -2, 0, 1, 4, 1, 8, mode, [9.0]).view(-1).tolist() == [float(v) for v in want]
        assert ref.oracle(frame, 0, -2, 0, 1, 4, 1, 8, mode, [9.0], (2, 0, 2, 0)).view(-1).tolist() == [float(v) for v in want]
    assert F.pad(x.view(1, 1, 4), (2, 2), mode="reflect").view(-1).tolist() == [3, 2, 1, 2, 3, 4, 3, 2]
    with pytest.raises(RuntimeError):
        F.pad(x.view(1, 1, 4), (4, 0), mode="reflect")            # reflect refuses a pad >= the dimension
    assert ref.pad_limit("reflect", 4) == 3 and ref.pad_limit("symmetric", 4) == 4 and ref.pad_limit("edge", 4) is None


CASES = ref.cases()


def test_every_listed_geometry_is_covered_by_the_modes_that_take_it():
    assert len(ref.GEOMETRIES) == 10
    per_mode = {m: sum(1 for _, _, mode, _ in CASES if mode == m) for m in ref.MODES}
    assert per_mode == {"constant": 10, "edge": 10, "reflect": 9, "symmetric": 9}
    limit = {mode: pads for _, g, mode, pads in CASES if g[4] == "limit"}
    assert limit["reflect"] == (3, 4, 3, 4) and limit["symmetric"] == (4, 5, 4, 5)


@pytest.mark.parametrize("geometry,mode,pads", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_restatement_is_torchs_own_padding(geometry, mode, pads):
    """Full extents and a mixed one per geometry: every corner row of the kernel tests, bitwise."""
    Hs, Ws, th, tw, _ = geometry
    frame = torch.randn((2, Hs, Ws), generator=_gen(Hs * 7 + tw))
    fill = [0.25, -1.5]
    for h, w in {(Hs, Ws), ref_extent(geometry, mode, pads)}:
        for top, left, flip, _, _ in ref.corner_rows(h, w, th, tw, pads).tolist():
            got = ref.window(frame, top, left, flip, h, w, th, tw, mode, fill)
            assert torch.equal(got, ref.oracle(frame, top, left, flip, h, w, th, tw, mode, fill, pads)), (top, left, flip, h, w)


def ref_extent(geometry, mode, pads):
    """A smaller valid extent the pads and the crop still allow (the full one where none does)."""
    Hs, Ws, th, tw, _ = geometry
    pl, pt, pr, pb = pads
    slack = {"reflect": 1, "symmetric": 0}.get(mode)
    h = max(Hs - 2, th - pt - pb, 1, 0 if slack is None else max(pt, pb) + slack)
    w = max(Ws - 3, tw - pl - pr, 1, 0 if slack is None else max(pl, pr) + slack)
    return min(h, Hs), min(w, Ws)


# ---------------------------------------------------------------------------------------------- the spec
def test_spec_is_a_class_of_its_own():
    from clsurvey_amd.data import PAD_MODES, RandomCropFlip, RandomPadCropFlip, RandomResizedCropFlip
    s = RandomPadCropFlip((32, 32), 4)
    assert (s.size, s.padding, s.fill, s.padding_mode, s.p, s.extents) == ((32, 32), (4, 4, 4, 4), 0, "constant", 0.5, None)
    assert not isinstance(s, (RandomCropFlip, RandomResizedCropFlip)) and not issubclass(RandomPadCropFlip, RandomCropFlip)
    assert not isinstance(RandomCropFlip((32, 32)), RandomPadCropFlip) and not isinstance(RandomResizedCropFlip((8, 8)), RandomPadCropFlip)
    assert RandomPadCropFlip((8, 8), (1, 2)).padding == (1, 2, 1, 2)               # (left/right, top/bottom)
    assert RandomPadCropFlip((8, 8), [1, 2, 3, 0]).padding == (1, 2, 3, 0)         # (left, top, right, bottom)
    assert RandomPadCropFlip((8, 8), (5,)).padding == (5, 5, 5, 5) and RandomPadCropFlip((8, 8), 0).padding == (0, 0, 0, 0)
    assert PAD_MODES == ("constant", "edge", "reflect", "symmetric") == ref.MODES
    assert repr(RandomPadCropFlip((8, 7), (1, 2), fill=(0.5, 0.0, 1.0), padding_mode="reflect", p=0.25, extents=torch.tensor([[9, 9]]))) == \
        "RandomPadCropFlip(size=(8, 7), padding=(1, 2, 1, 2), fill=(0.5, 0.0, 1.0), padding_mode='reflect', p=0.25, extents=[1][2])"
    assert repr(s) == "RandomPadCropFlip(size=(32, 32), padding=(4, 4, 4, 4), fill=0, padding_mode='constant', p=0.5)"
    back = pickle.loads(pickle.dumps(RandomPadCropFlip((8, 7), (1, 2, 3, 0), [1, 2, 3], "symmetric", 0.25, torch.tensor([[9, 9]]))))
    assert (back.size, back.padding, back.fill, back.padding_mode, back.p, back.extents.tolist()) == \
        ((8, 7), (1, 2, 3, 0), (1, 2, 3), "symmetric", 0.25, [[9, 9]])
    for bad in (dict(size=(0, 8), padding=1), dict(size=(8, 8), padding=1, p=1.5), dict(size=(8, 8), padding=-1),
                dict(size=(8, 8), padding=(1, -2)), dict(size=(8, 8), padding=(1, 2, 3)), dict(size=(8, 8), padding=()),
                dict(size=(8, 8), padding=1.5), dict(size=(8, 8), padding=(1, 2.0)), dict(size=(8, 8), padding=40000),
                dict(size=(8, 8), padding=1, padding_mode="wrap"), dict(size=(8, 8), padding=1, padding_mode="replicate"),
                dict(size=(8, 8), padding=1, fill="grey"), dict(size=(8, 8), padding=1, fill=()),
                dict(size=(8, 8), padding=1, fill=(0.0, float("nan"))), dict(size=(8, 8), padding=1, fill=None)):
        with pytest.raises(ValueError):
            RandomPadCropFlip(**bad)


def test_fill_is_checked_against_the_dataset_it_is_attached_to():
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip, TensorTaskDataset
    x, xb, y = torch.zeros((4, 3, 8, 8)), torch.zeros((4, 3, 8, 8), dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    mean, std = [0.5] * 3, [0.25] * 3
    assert RandomPadCropFlip((8, 8), 2, fill=0.5).fill_values(3) == (0.5, 0.5, 0.5)
    assert RandomPadCropFlip((8, 8), 2, fill=(1, 2, 3)).fill_values(3, byte=True) == (1, 2, 3)
    TensorTaskDataset(x, y, ["0"], transform=RandomPadCropFlip((8, 8), 2, fill=(0.1, 0.2, 0.3)))
    ByteTaskDataset(xb, y, ["0"], mean, std, transform=RandomPadCropFlip((8, 8), 2, fill=(0, 128, 255)))
    ByteTaskDataset(xb, y, ["0"], mean, std, transform=RandomPadCropFlip((8, 8), 2, fill=7))
    with pytest.raises(ValueError, match="2 fill values for 3 channels"):
        TensorTaskDataset(x, y, ["0"], transform=RandomPadCropFlip((8, 8), 2, fill=(0.1, 0.2)))
    for fill in (0.5, 256, -1, (0, 1, 2.0)):
        with pytest.raises(ValueError, match="ints in 0..255"):
            ByteTaskDataset(xb, y, ["0"], mean, std, transform=RandomPadCropFlip((8, 8), 2, fill=fill))
    with pytest.raises(ValueError):
        TensorTaskDataset(x, y, ["0"], transform=RandomPadCropFlip((8, 8), 2, extents=torch.full((3, 2), 8)))


# ---------------------------------------------------------------------------------------------- the draws
def test_zero_pads_draw_what_the_plain_crop_draws():
    from clsurvey_amd.data import RandomCropFlip, RandomPadCropFlip, draw_crop_flip, draw_pad_crop_flip
    ext = torch.stack([torch.randint(16, 21, (50,), generator=_gen(1)), torch.randint(12, 25, (50,), generator=_gen(2))], 1)
    order = torch.randperm(50, generator=_gen(3))
    for extents, frame, perm in ((None, (20, 24), None), (ext, (20, 24), None), (ext, (20, 24), order)):
        a = draw_pad_crop_flip(50, RandomPadCropFlip((16, 12), 0, p=0.3, extents=extents), frame, _gen(9), order=perm)
        b = draw_crop_flip(50, RandomCropFlip((16, 12), p=0.3, extents=extents), frame, _gen(9), order=perm)
        assert a.dtype == torch.int32 and tuple(a.shape) == (50, 5) and torch.equal(a[:, :3], b)
        want = torch.tensor([frame] * 50) if extents is None else (ext if perm is None else ext[perm])
        assert torch.equal(a[:, 3:].long(), want)


def test_every_corner_of_both_ranges_is_drawn_and_nothing_outside():
    from clsurvey_amd.data import RandomPadCropFlip, draw_pad_crop_flip
    spec = RandomPadCropFlip((8, 8), (1, 2, 3, 0))                                 # pl, pt, pr, pb
    g = _gen(11)
    t = draw_pad_crop_flip(4096, spec, (8, 8), g)
    # top in [-pt, h + pb - th] = [-2, 0], left in [-pl, w + pr - tw] = [-1, 3]
    assert sorted(set(t[:, 0].tolist())) == [-2, -1, 0] and sorted(set(t[:, 1].tolist())) == [-1, 0, 1, 2, 3]
    assert sorted(set(t[:, 2].tolist())) == [0, 1] and set(map(tuple, t[:, 3:].tolist())) == {(8, 8)}
    # the generator ends where one rand((n, 3), float64) call leaves it, and the table is that call's
    g2 = _gen(11)
    u = torch.rand((4096, 3), generator=g2, dtype=torch.float64)
    assert torch.equal(g.get_state(), g2.get_state())
    assert torch.equal(t[:, 0].long(), torch.minimum((u[:, 0] * 3).floor().long(), torch.tensor(2)) - 2)
    assert torch.equal(t[:, 1].long(), torch.minimum((u[:, 1] * 5).floor().long(), torch.tensor(4)) - 1)
    assert torch.equal(t[:, 2].long(), (u[:, 2] < 0.5).long())
    assert torch.equal(t, draw_pad_crop_flip(4096, spec, (8, 8), _gen(11)))
    assert tuple(draw_pad_crop_flip(0, spec, (8, 8), _gen(1)).shape) == (0, 5)
    # a crop larger than the frame is legal when the padded image holds it; with no freedom the corner is (-pt, -pl)
    t = draw_pad_crop_flip(7, RandomPadCropFlip((12, 12), 2, p=0.0), (8, 8), _gen(2))
    assert t.tolist() == [[-2, -2, 0, 8, 8]] * 7


def test_draw_raises_on_what_the_gather_would_call_a_bad_row():
    from clsurvey_amd.data import RandomPadCropFlip, draw_pad_crop_flip
    with pytest.raises(ValueError, match="smaller than the crop"):
        draw_pad_crop_flip(3, RandomPadCropFlip((13, 8), 2), (8, 8), _gen(1))
    with pytest.raises(ValueError, match="smaller than the crop"):
        draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), 1, extents=torch.tensor([[8, 8], [8, 5], [8, 8]])), (8, 8), _gen(1))
    with pytest.raises(ValueError, match="exceeds the stored frame"):
        draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), 1, extents=torch.tensor([[8, 8], [9, 8], [8, 8]])), (8, 8), _gen(1))
    with pytest.raises(ValueError, match="empty extent"):
        draw_pad_crop_flip(2, RandomPadCropFlip((4, 4), 4, extents=torch.tensor([[8, 8], [0, 8]])), (8, 8), _gen(1))
    with pytest.raises(ValueError, match="extents for"):
        draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), 1, extents=torch.full((2, 2), 8)), (8, 8), _gen(1))
    # the mode's limit, judged on the smallest extent: reflect takes extent - 1, symmetric extent, constant and edge anything
    small = torch.tensor([[8, 8], [8, 4], [8, 8]])
    draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), (3, 7), padding_mode="reflect", extents=small), (8, 8), _gen(1))
    draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), (4, 8), padding_mode="symmetric", extents=small), (8, 8), _gen(1))
    for mode, pad in (("reflect", (4, 1)), ("reflect", (2, 8)), ("symmetric", (5, 1)), ("symmetric", (2, 9))):
        with pytest.raises(ValueError, match="takes pads up to"):
            draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), pad, padding_mode=mode, extents=small), (8, 8), _gen(1))
    for mode in ("constant", "edge"):
        draw_pad_crop_flip(3, RandomPadCropFlip((8, 8), 40, padding_mode=mode, extents=small), (8, 8), _gen(1))


@pytest.mark.parametrize("shuffle", [True, False])
def test_loader_with_the_spec_consumes_the_global_generator_like_a_plain_one(shuffle):
    from clsurvey_amd.data import DeviceLoader, RandomPadCropFlip, TensorTaskDataset, draw_pad_crop_flip
    x, y = torch.randn((24, 3, 16, 16), generator=_gen(5)), torch.arange(24) % 4
    names = [str(c) for c in range(4)]
    aug = TensorTaskDataset(x, y, names, transform=RandomPadCropFlip((16, 16), 4, padding_mode="reflect"))
    plain = TensorTaskDataset(x, y, names)
    a, b = DeviceLoader(aug, 7, shuffle, device="cpu"), DeviceLoader(plain, 7, shuffle, device="cpu")
    assert tuple(a.x.shape) == (0, 3, 16, 16) and tuple(a.frames[0].shape) == (24, 3, 16, 16) and len(a) == len(b) == 4
    assert a.transform is aug.transform and a.geometry == (3, 16, 16, 16, 16) and b.transform is None
    torch.manual_seed(5)
    pa = a.order()
    sa = torch.get_rng_state()
    torch.manual_seed(5)
    pb = b.order()
    assert torch.equal(sa, torch.get_rng_state())
    assert (pa is None and pb is None) if not shuffle else torch.equal(pa, pb)
    t1 = a.epoch_params(pa)
    assert torch.equal(sa, torch.get_rng_state())                                   # (the table comes from a private generator)
    assert tuple(t1.shape) == (24, 5) and torch.equal(t1, draw_pad_crop_flip(24, aug.transform, (16, 16), _gen(a.base_seed), order=pa))
    # a crop larger than the frame passes the loader when the padded image holds it, and is refused for the unpadded spec
    big = TensorTaskDataset(x, y, names, transform=RandomPadCropFlip((20, 20), 2))
    assert tuple(DeviceLoader(big, 7, shuffle, device="cpu").x.shape) == (0, 3, 20, 20)


# ---------------------------------------------------------------------------------------------- merging, decoded()
def test_tasks_of_one_list_carry_equal_padding_mode_and_fill():
    from clsurvey_amd.data import RandomCropFlip, RandomPadCropFlip, TensorTaskDataset, _respec, _spec_key, _transform_of, merged_transform
    x, y = torch.zeros((6, 3, 16, 16)), torch.zeros(6, dtype=torch.int64)

    def with_spec(spec):
        return TensorTaskDataset(x, y, ["0"], transform=spec)

    base = dict(size=(16, 16), padding=4, fill=0.0, padding_mode="constant", p=0.5)
    aug = with_spec(RandomPadCropFlip(**base))
    assert _transform_of(aug) is aug.transform
    t = merged_transform([aug, with_spec(RandomPadCropFlip(**base))])
    assert isinstance(t, RandomPadCropFlip) and (t.size, t.padding, t.fill, t.padding_mode, t.p, t.extents) == \
        ((16, 16), (4, 4, 4, 4), 0.0, "constant", 0.5, None)
    for other in (dict(size=(16, 12)), dict(padding=3), dict(padding=(4, 4, 4, 3)), dict(fill=1.0), dict(fill=(0.0, 0.0, 1.0)),
                  dict(padding_mode="edge"), dict(p=0.25)):
        with pytest.raises(ValueError):
            merged_transform([aug, with_spec(RandomPadCropFlip(**dict(base, **other)))])
    with pytest.raises(ValueError):
        merged_transform([aug, with_spec(None)])
    with pytest.raises(ValueError):                                                 # two classes of equal size and p
        merged_transform([aug, with_spec(RandomCropFlip((16, 16)))])
    with pytest.raises(ValueError):
        merged_transform([with_spec(RandomCropFlip((16, 16))), aug])
    ext = with_spec(RandomPadCropFlip(extents=torch.full((6, 2), 14), **base))
    t = merged_transform([aug, ext])
    assert isinstance(t, RandomPadCropFlip) and t.extents[0].tolist() == [16, 16] and t.extents[6].tolist() == [14, 14]
    r = _respec(ext.transform, torch.full((2, 2), 9))
    assert isinstance(r, RandomPadCropFlip) and _spec_key(r) == _spec_key(ext.transform) and r.extents.tolist() == [[9, 9]] * 2


def test_decoded_translates_the_fill_through_the_table():
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip, norm_lut
    xb = torch.randint(0, 256, (5, 3, 8, 8), generator=_gen(4), dtype=torch.uint8)
    y = torch.zeros(5, dtype=torch.int64)
    mean, std = torch.tensor([0.4, 0.5, 128.0 / 255]), torch.tensor([0.2, 0.25, 48.0 / 255])
    lut = norm_lut(mean, std)
    spec = RandomPadCropFlip((8, 8), (1, 2), fill=(3, 200, 128), padding_mode="constant", p=0.25, extents=torch.full((5, 2), 7))
    d = ByteTaskDataset(xb, y, ["0"], mean, std, transform=spec).decoded()
    t = d.transform
    assert isinstance(t, RandomPadCropFlip) and t is not spec and spec.fill == (3, 200, 128)
    assert (t.size, t.padding, t.padding_mode, t.p) == ((8, 8), (1, 2, 1, 2), "constant", 0.25) and torch.equal(t.extents, spec.extents)
    assert torch.equal(torch.tensor(t.fill, dtype=torch.float32), torch.stack([lut[0, 3], lut[1, 200], lut[2, 128]]))
    assert t.fill[2] == 0.0                                                         # byte 128 under mean 128 / 255 is exactly 0
    assert d.x.dtype == torch.float32 and torch.equal(d.x[:, 1], lut[1][xb[:, 1].long()])
    scalar = ByteTaskDataset(xb, y, ["0"], mean, std, transform=RandomPadCropFlip((8, 8), 1, fill=9)).decoded().transform
    assert torch.equal(torch.tensor(scalar.fill, dtype=torch.float32), lut[:, 9])
    # a split without the spec hands over what it carries
    assert ByteTaskDataset(xb, y, ["0"], mean, std).decoded().transform is None


# ---------------------------------------------------------------------------------------------- the ABI
def test_argument_errors_do_not_need_a_device():
    import ctypes as C
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 64)()
    one = C.addressof(buf)                                        # any non-null pointer: never dereferenced on these paths
    for name, lut in (("clhip_gather_tasks_pad_crop_flip", ()), ("clhip_gather_tasks_pad_crop_flip_u8", (one,))):
        assert name in _lib.SIGNATURES
        fn = getattr(L, name)

        def f(tasks=one, T=3, Cc=3, Hs=20, Ws=20, th=16, tw=16, mode=0, pads=(4, 4, 4, 4), fill=one, idx=one, params=one, B=4,
              x_out=one, labels=one, lut=lut):
            return fn(tasks, T, Cc, Hs, Ws, th, tw, mode, *pads, fill, *lut, idx, params, B, x_out, labels, None)

        assert f(B=0) == 0                                                           # nothing to do
        assert f(B=0, th=30, tw=28) == 0                                             # a crop larger than the frame: no error
        # null pointers
        for kw in (dict(tasks=None), dict(fill=None), dict(idx=None), dict(params=None), dict(x_out=None), dict(labels=None)):
            assert f(**kw) == -1, kw
        if lut:
            assert f(lut=(None,)) == -1
        # mode outside 0..3
        assert f(mode=-1) == -1 and f(mode=4) == -1 and all(f(mode=m, B=0) == 0 for m in range(4))
        # a negative pad, a pad above 32767
        for i in range(4):
            for v in (-1, 32768):
                pads = [4, 4, 4, 4]
                pads[i] = v
                assert f(pads=pads) == -1, pads
        assert f(pads=(32767, 0, 32767, 0), B=0) == 0
        # sizes and the task count
        for kw in (dict(th=0), dict(tw=0), dict(Cc=0), dict(Hs=0), dict(Ws=0), dict(T=0), dict(T=65), dict(B=-1), dict(B=70000)):
            assert f(**kw) == -1, kw
        assert f(T=64, B=0) == 0


def test_ops_refuse_cpu_tensors():
    from clsurvey_amd import ops
    table = torch.zeros((1, 4), dtype=torch.int64)
    idx = torch.zeros((2,), dtype=torch.int64)
    params = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device tensors"):
        ops.gather_tasks_pad_crop_flip(table, (3, 20, 20, 16, 16), "constant", (4, 4, 4, 4), torch.zeros(3), idx, params)
    with pytest.raises(RuntimeError, match="HIP device tensors"):
        ops.gather_tasks_pad_crop_flip_u8(table, (3, 20, 20, 16, 16), 2, (4, 4, 4, 4), torch.zeros(3), torch.zeros((3, 256)), idx, params)
    assert ops.PAD_MODES == ref.MODES


# ---------------------------------------------------------------------------------------------- refusal
def _padded_split(byte=False):
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip, TensorTaskDataset
    y = torch.arange(8) % 2
    if byte:
        return ByteTaskDataset(torch.zeros((8, 3, 12, 12), dtype=torch.uint8), y, ["0", "1"], [0.5] * 3, [0.25] * 3,
                               transform=RandomPadCropFlip((12, 12), 2, fill=128))
    return TensorTaskDataset(torch.zeros((8, 3, 12, 12)), y, ["0", "1"], transform=RandomPadCropFlip((12, 12), 2))


def test_rehearsal_entry_refuses_the_spec(tmp_path):
    """GEM and R-PM / R-FM replay stored frames without padding: a train split with the padded spec is an error, raised before
    any loader or device is touched."""
    from clsurvey_amd.methods import gem_main
    prev = os.path.join(str(tmp_path), "prev.pth.tar")
    torch.save({}, prev)
    for method in ("gem", "baseline_rehearsal_full_mem", "baseline_rehearsal_partial_mem"):
        for byte, extra in ((False, {}), (True, {}), (True, dict(exemplar_dtype="uint8")), (False, dict(exemplar_resized=True))):
            train = _padded_split(byte)
            args = dict(task_name="2", task_count=2, prev_model_path=prev, n_outputs=4, method=method, n_memories=4, n_tasks=2,
                        dataset_path={"train": train, "val": train, "test": train}, postprocess=False, is_scratch_model=False, **extra)
            with pytest.raises(NotImplementedError, match="padded replay is not built"):
                gem_main.main(args, [2, 2], device="cpu")


def test_icarl_entry_refuses_the_spec(tmp_path):
    from clsurvey_amd.methods import icarl_main
    path = os.path.join(str(tmp_path), "SI_first_task.pth.tar")
    with open(path, "wb") as f:
        f.write(b"x")                                              # (must exist; the refusal comes before it is read)
    for byte, extra in ((False, {}), (False, dict(exemplar_frames=True)), (True, dict(exemplar_frames=True, exemplar_dtype="uint8")),
                        (False, dict(exemplar_frames=True, exemplar_resized=True))):
        train = _padded_split(byte)
        args = dict(task_name="1", task_count=1, prev_model_path=path, save_path=os.path.join(str(tmp_path), "out"), n_outputs=4,
                    method="icarl", postprocess=True, is_scratch_model=True, n_memories=4, n_tasks=2, batch_size=4,
                    dataset_path={"train": train, "val": train}, **extra)
        with pytest.raises(NotImplementedError, match="padded replay is not built"):
            icarl_main.main(args, [2, 2], device="cpu")


# ---------------------------------------------------------------------------------------------- the task sequence
def _seq(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    return SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                                 name="aug2", **kw)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("u8", [False, True], ids=["float", "u8_frames"])
def test_rnd_pad_zero_writes_what_it_always_wrote(tmp_path, u8):
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    with_flag, without = _seq(a, rnd_pad=0, pad_mode="reflect", u8_frames=u8), _seq(b, u8_frames=u8)
    base = {"sizes": [24, 8, 8], "classes": 4, "hw": 16, "seed": 7001, "noise": 0.4, "kind": "protos", "blobs": None}
    assert with_flag.spec("1") == without.spec("1") == dict(base, **({"u8_frames": True} if u8 else {}))
    pa, pb = with_flag.get_task_dataset_path("1", rnd_transform=True), without.get_task_dataset_path("1", rnd_transform=True)
    assert os.path.basename(pa) == os.path.basename(pb) == "task_1.pth.tar"
    assert _bytes(pa) == _bytes(pb) and _bytes(pa[:-8] + ".spec.json") == _bytes(pb[:-8] + ".spec.json")
    assert sorted(os.listdir(os.path.dirname(pa))) == ["task_1.pth.tar", "task_1.spec.json"]
    # and with a margin of another kind the sidecar has no new key
    assert not {"rnd_pad", "pad_mode"} & set(_seq(a, rnd_margin=4).spec("1", True))


@pytest.mark.parametrize("u8", [False, True], ids=["float", "u8_frames"])
def test_rnd_pad_writes_two_files_of_the_same_images(tmp_path, u8):
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip
    ds = _seq(str(tmp_path), rnd_pad=4, pad_mode="symmetric", u8_frames=u8)
    raw_path = ds.get_task_dataset_path("2")
    aug_path = ds.get_task_dataset_path("2", rnd_transform=True)
    assert os.path.basename(raw_path) == "task_2.pth.tar" and os.path.basename(aug_path) == "task_2_rndtrans.pth.tar"
    want = {"sizes": [24, 8, 8], "classes": 4, "hw": 16, "seed": 7002, "noise": 0.4, "kind": "protos", "blobs": None, "rnd_pad": 4,
            "pad_mode": "symmetric"}
    if u8:
        want["u8_frames"] = True
    assert ds.spec("2") == want and ds.spec("2", True) == dict(want, rnd_transform=True) and ds.input_size == (16, 16)
    raw, aug = torch.load(raw_path, weights_only=False), torch.load(aug_path, weights_only=False)
    t = aug["train"].transform
    assert isinstance(t, RandomPadCropFlip)
    assert (t.size, t.padding, t.padding_mode, t.p, t.extents) == ((16, 16), (4, 4, 4, 4), "symmetric", 0.5, None)
    assert (t.fill == 128 and isinstance(t.fill, int)) if u8 else (t.fill == 0.0 and isinstance(t.fill, float))
    for split in ("train", "val", "test"):                                          # no margin: both files hold the same images
        assert torch.equal(raw[split].x, aug[split].x) and torch.equal(raw[split].y, aug[split].y)
        assert isinstance(raw[split], ByteTaskDataset) == u8 == isinstance(aug[split], ByteTaskDataset)
        assert raw[split].transform is None and (aug[split].transform is None) == (split != "train")
    assert tuple(aug["train"].x.shape) == (24, 3, 16, 16)
    if u8:
        assert aug["train"].decoded().transform.fill == (0.0, 0.0, 0.0)             # byte 128 decodes to exactly 0.0
    # the images are those of the sequence without the option
    plain = torch.load(_seq(os.path.join(str(tmp_path), "plain"), u8_frames=u8).get_task_dataset_path("2"), weights_only=False)
    assert torch.equal(plain["train"].x, aug["train"].x)
    assert sorted(os.listdir(os.path.dirname(raw_path))) == ["task_2.pth.tar", "task_2.spec.json", "task_2_rndtrans.pth.tar",
                                                             "task_2_rndtrans.spec.json"]
    always = _seq(str(tmp_path), rnd_pad=4, pad_mode="symmetric", u8_frames=u8, rnd_always=True)
    assert always.get_task_dataset_path("2", rnd_transform=False) == aug_path
    # another mode or pad is another spec: an error, not a hit
    with pytest.raises(RuntimeError):
        _seq(str(tmp_path), rnd_pad=4, pad_mode="reflect", u8_frames=u8).get_task_dataset_path("2", True)
    with pytest.raises(RuntimeError):
        _seq(str(tmp_path), rnd_pad=2, pad_mode="symmetric", u8_frames=u8).get_task_dataset_path("2")
    for bad in (dict(rnd_pad=4, rnd_margin=4), dict(rnd_pad=4, rnd_resized=4), dict(rnd_pad=-1), dict(rnd_pad=4, pad_mode="wrap")):
        with pytest.raises(ValueError):
            _seq(str(tmp_path), **bad)
    assert _seq(str(tmp_path), rnd_pad=4).pad_mode == "constant"


def test_driver_flags(tmp_path):
    from clsurvey_amd.framework import driver
    common = ["small_VGG9_cl_128_128", "--method_name", "EWC", "--results_root", str(tmp_path)]
    syn = ["--synthetic", "2,4,160,40,40,32"]
    for extra in (["--rnd_pad", "4"],                                               # belongs to --synthetic
                  syn + ["--rnd_pad", "4", "--rnd_margin", "4"], syn + ["--rnd_pad", "4", "--rnd_resized", "4"],
                  syn + ["--pad_mode", "reflect"], syn + ["--rnd_pad", "0", "--pad_mode", "edge"], syn + ["--rnd_pad", "-1"],
                  syn + ["--rnd_pad", "4", "--pad_mode", "wrap"],
                  # a padded split does not satisfy the exemplar flags
                  syn + ["--rnd_pad", "4", "--icarl_frames"], syn + ["--rnd_pad", "4", "--resized_exemplars"],
                  syn + ["--rnd_pad", "4", "--u8_frames", "--u8_exemplars"]):
        with pytest.raises(SystemExit):
            driver.main(common + extra)
    assert not os.path.exists(os.path.join(str(tmp_path), "data"))
    args = driver.build_parser().parse_args(common)
    assert args.rnd_pad == 0 and args.pad_mode is None
    args = driver.build_parser().parse_args(common + syn + ["--rnd_pad", "4", "--pad_mode", "symmetric", "--u8_frames"])
    assert args.rnd_pad == 4 and args.pad_mode == "symmetric" and args.u8_frames
