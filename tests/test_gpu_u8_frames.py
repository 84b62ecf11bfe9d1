"""Byte frames on the GPU: the three ..._u8 gathers against their fp32 entries run on the decoded frames, the loaders over a
ByteTaskDataset against the loaders over its `.decoded()`, finetune / R-PM / iCaRL herding on byte splits against the decoded
splits, and `--u8_frames` through the driver.  Every comparison of values is torch.equal on the int32 view: no tolerance."""
import functools
import os
import random
import sys
import types
from itertools import accumulate

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # distinct per channel


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lut(C):
    from clsurvey_amd.data import norm_lut
    return norm_lut(torch.tensor(MEAN[:C]), torch.tensor(STD[:C]))


def _decode(x, lut):
    """The meaning of byte frames [n][C][H][W] on the CPU: lut[c][x]."""
    return torch.stack([lut[c][x[:, c].long()] for c in range(x.shape[1])], 1)


@functools.lru_cache(maxsize=None)
def _tasks(T, C, Hs, Ws, odd_base=False):
    """T = 1 (13 frames) or 3 (5, 1, 7 frames: every task boundary, label shifts) tasks of byte frames, frame 0 = arange(256)
    repeated (every table entry of every channel is used), with their decoded twins; all on the device, made once.
    odd_base: every frame tensor starts one byte into its storage."""
    gen = torch.Generator().manual_seed(1000 * T + 100 * C + Hs + Ws)
    sizes, ncls = ([5, 1, 7], [3, 2, 4]) if T == 3 else ([13], [9])
    xs = [torch.randint(0, 256, (n, C, Hs, Ws), generator=gen, dtype=torch.uint8) for n in sizes]
    xs[0][0] = torch.arange(256, dtype=torch.uint8).repeat((C * Hs * Ws + 255) // 256)[:C * Hs * Ws].view(C, Hs, Ws)
    ys = [torch.randint(0, k, (n,), generator=gen) for n, k in zip(sizes, ncls)]
    lut = _lut(C)
    fs = [_decode(x, lut).to(DEV) for x in xs]
    if odd_base:
        bufs = [torch.empty((x.numel() + 1,), dtype=torch.uint8, device=DEV) for x in xs]
        bx = [b[1:].view(x.shape).copy_(x) for b, x in zip(bufs, xs)]
        assert all(v.data_ptr() % 2 == 1 and v.is_contiguous() for v in bx)
    else:
        bx = [x.to(DEV) for x in xs]
    return dict(bx=bx, fs=fs, ys=[y.to(DEV) for y in ys], cum=list(accumulate(sizes)), shifts=[0] + list(accumulate(ncls))[:-1],
                lut=lut.to(DEV), labels=torch.cat([y + s for y, s in zip(ys, [0] + list(accumulate(ncls))[:-1])]))


def _tables(t):
    from clsurvey_amd import ops
    return ops.task_table(t["bx"], t["ys"], t["cum"], t["shifts"], DEV), ops.task_table(t["fs"], t["ys"], t["cum"], t["shifts"], DEV)


def _idx(total, B, gen):
    """B = 1: the last sample.  Otherwise every sample of every task once, then drawn ones."""
    if B == 1:
        return torch.tensor([total - 1])
    return torch.cat([torch.arange(total), torch.randint(0, total, (B - total,), generator=gen)])


def _same(got, want, labels, idx):
    assert got[0].dtype == torch.float32 and got[0].shape == want[0].shape
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])
    assert torch.equal(got[1].cpu(), labels[idx])


# ---------------------------------------------------------------------------------------------- kernels
ROWS = [(1, 5, 7), (2, 3, 3), (3, 8, 8), (3, 72, 72)]
CROPS = [(1, 9, 11, 5, 6), (3, 10, 12, 8, 8), (3, 13, 13, 8, 8), (2, 8, 8, 8, 8), (3, 72, 72, 64, 64)]
RESIZED = [(1, 5, 7, 8, 8), (3, 40, 33, 8, 8), (2, 9, 9, 4, 12), (3, 64, 64, 56, 56), (2, 64, 64, 8, 8), (3, 12, 10, 5, 7)]


def _crop_params(Hs, Ws, th, tw, B, gen):
    """Offsets 0 and the maximum in both axes under both flips, then drawn rows."""
    from clsurvey_amd.data import RandomCropFlip, draw_crop_flip
    mt, ml = Hs - th, Ws - tw
    hand = torch.tensor([[0, 0, 0], [mt, ml, 1], [0, ml, 1], [mt, 0, 0], [mt // 2, min(1, ml), 1], [min(1, mt), ml // 2, 0],
                         [mt, min(3, ml), 1], [0, 0, 1]], dtype=torch.int32)
    if B == 1:
        return hand[1:2].clone()
    return torch.cat([hand, draw_crop_flip(B - len(hand), RandomCropFlip((th, tw)), (Hs, Ws), gen)])


def _resized_params(Hs, Ws, th, tw, B, gen):
    """1 x 1 windows in two corners, the whole frame under both flips, a window touching each border, then drawn rows."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    h, w = max(1, (2 * Hs) // 3), max(1, (2 * Ws) // 3)
    hand = torch.tensor([[0, 0, 1, 1, 0], [Hs - 1, Ws - 1, 1, 1, 1], [0, 0, Hs, Ws, 0], [0, 0, Hs, Ws, 1], [0, (Ws - w) // 2, h, w, 1],
                         [Hs - h, (Ws - w) // 2, h, w, 0], [(Hs - h) // 2, 0, h, w, 1], [(Hs - h) // 2, Ws - w, h, w, 0]], dtype=torch.int32)
    if B == 1:
        return hand[3:4].clone()
    return torch.cat([hand, draw_resized_crop_flip(B - len(hand), RandomResizedCropFlip((th, tw)), (Hs, Ws), gen)])


@pytest.mark.parametrize("C,H,W", ROWS, ids=["%dx%dx%d" % r for r in ROWS])
def test_plain_gather_is_the_fp32_gather_of_the_decoded_rows(C, H, W):
    """Scalar stores with an odd plane / a row of 18 elements whose planes of 9 are crossed inside a block / float4 stores /
    a row of three 16 KB segments, one per channel."""
    from clsurvey_amd import ops
    for T in (1, 3):
        t = _tasks(T, C, H, W)
        tb, tf = _tables(t)
        for B in (1, 37):
            idx = _idx(t["cum"][-1], B, torch.Generator().manual_seed(B + T))
            got = ops.gather_tasks_u8(tb, C, H * W, t["lut"], idx.to(DEV))
            want = ops.gather_tasks(tf, C * H * W, idx.to(DEV))
            assert tuple(got[0].shape) == (B, C * H * W)
            _same(got, want, t["labels"], idx)


def test_plain_gather_crosses_planes_inside_a_float4():
    """C = 2, plane of 6: row_elems = 12 takes the float4 stores and the second vector holds bytes of both channels."""
    from clsurvey_amd import ops
    t = _tasks(3, 2, 2, 3)
    tb, tf = _tables(t)
    idx = torch.arange(13)
    _same(ops.gather_tasks_u8(tb, 2, 6, t["lut"], idx.to(DEV)), ops.gather_tasks(tf, 12, idx.to(DEV)), t["labels"], idx)


@pytest.mark.parametrize("geo", CROPS, ids=["%dx%dx%d_to_%dx%d" % g for g in CROPS])
def test_crop_flip_is_the_fp32_entry_on_the_decoded_frames(geo):
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = geo
    for T in (1, 3):
        t = _tasks(T, C, Hs, Ws)
        tb, tf = _tables(t)
        for B in (1, 37):
            gen = torch.Generator().manual_seed(B + T)
            idx, params = _idx(t["cum"][-1], B, gen), _crop_params(Hs, Ws, th, tw, B, gen)
            assert B == 1 or set(params[:, 2].tolist()) == {0, 1}
            got = ops.gather_tasks_crop_flip_u8(tb, geo, t["lut"], idx.to(DEV), params.to(DEV))
            want = ops.gather_tasks_crop_flip(tf, geo, idx.to(DEV), params.to(DEV))
            assert tuple(got[0].shape) == (B, C, th, tw)
            _same(got, want, t["labels"], idx)


@pytest.mark.parametrize("geo", RESIZED, ids=["%dx%dx%d_to_%dx%d" % g for g in RESIZED])
def test_resized_crop_flip_is_the_fp32_entry_on_the_decoded_frames(geo):
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = geo
    for T in (1, 3):
        t = _tasks(T, C, Hs, Ws)
        tb, tf = _tables(t)
        for B in (1, 37):
            gen = torch.Generator().manual_seed(B + T)
            idx, params = _idx(t["cum"][-1], B, gen), _resized_params(Hs, Ws, th, tw, B, gen)
            assert B == 1 or set(params[:, 4].tolist()) == {0, 1}
            got = ops.gather_tasks_resized_crop_flip_u8(tb, geo, t["lut"], idx.to(DEV), params.to(DEV))
            want = ops.gather_tasks_resized_crop_flip(tf, geo, idx.to(DEV), params.to(DEV))
            assert tuple(got[0].shape) == (B, C, th, tw)
            _same(got, want, t["labels"], idx)


def _launch_pair(kind, t, geo, idx, params, **out):
    """(u8 entry on the bytes, fp32 entry on the decoded frames) of one of the three gathers."""
    from clsurvey_amd import ops
    tb, tf = _tables(t)
    idx = idx.to(DEV)
    if kind == "plain":
        C, H, W = geo[:3]
        return ops.gather_tasks_u8(tb, C, H * W, t["lut"], idx, **out), ops.gather_tasks(tf, C * H * W, idx)
    params = params.to(DEV)
    if kind == "crop":
        return ops.gather_tasks_crop_flip_u8(tb, geo, t["lut"], idx, params, **out), ops.gather_tasks_crop_flip(tf, geo, idx, params)
    return (ops.gather_tasks_resized_crop_flip_u8(tb, geo, t["lut"], idx, params, **out),
            ops.gather_tasks_resized_crop_flip(tf, geo, idx, params))


def _case(kind, geo, odd_base=False, T=3, B=37):
    C, Hs, Ws = geo[:3]
    t = _tasks(T, C, Hs, Ws, odd_base)
    gen = torch.Generator().manual_seed(B + T)
    idx = _idx(t["cum"][-1], B, gen)
    params = None if kind == "plain" else (_crop_params if kind == "crop" else _resized_params)(Hs, Ws, geo[3], geo[4], B, gen)
    return t, idx, params


@pytest.mark.parametrize("kind,geo", [("crop", (3, 13, 13, 8, 8)), ("resized", (3, 12, 10, 5, 7)), ("plain", (3, 8, 8)), ("plain", (3, 5, 7))],
                         ids=["crop_13x13_to_8x8", "resized_12x10_to_5x7", "plain_3x8x8", "plain_3x5x7"])
def test_frames_that_start_at_an_odd_address(kind, geo):
    """The frame tensors start one byte into their storage: a load wider than a byte is right only behind a test of the address
    (crop: float4 stores from lines of 13 bytes; plain 3x8x8: float4 stores, no source row 4-byte aligned)."""
    t, idx, params = _case(kind, geo, odd_base=True)
    got, want = _launch_pair(kind, t, geo, idx, params)
    _same(got, want, t["labels"], idx)


@pytest.mark.parametrize("kind,geo", [("plain", (3, 8, 8)), ("crop", (3, 10, 12, 8, 8)), ("resized", (3, 40, 33, 8, 8))],
                         ids=["plain", "crop", "resized"])
def test_unaligned_output_takes_the_plain_stores(kind, geo):
    """x_out 4 bytes off a 16-byte boundary at a shape that otherwise takes float4 stores: the same bytes, nothing before or
    after the buffer."""
    t, idx, params = _case(kind, geo)
    row = geo[0] * (geo[1] * geo[2] if kind == "plain" else geo[3] * geo[4])
    n = idx.shape[0] * row
    buf = torch.full((1 + n + 3,), -7.0, device=DEV)
    assert buf[1:].data_ptr() % 16 == 4
    got, want = _launch_pair(kind, t, geo, idx, params, x_out=buf[1:])
    assert torch.equal(_bits(buf[1:1 + n]), _bits(want[0].view(-1))) and torch.equal(got[1], want[1])
    assert float(buf[0]) == -7.0 and bool((buf[1 + n:] == -7.0).all())


@pytest.mark.parametrize("kind,geo", [("plain", (3, 72, 72)), ("crop", (3, 72, 72, 64, 64)), ("resized", (3, 64, 64, 56, 56))],
                         ids=["plain", "crop", "resized"])
def test_two_launches_are_bitwise_equal(kind, geo):
    t, idx, params = _case(kind, geo)
    a, _ = _launch_pair(kind, t, geo, idx, params)
    b, _ = _launch_pair(kind, t, geo, idx, params)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


def _bad_rows(kind):
    """(geometry, [(sample number, parameter row, good)]): the lists of tests/test_gpu_augment.py and
    tests/test_gpu_resized_crop.py; for the plain gather the sample numbers total, -1 and 2^40."""
    if kind == "plain":
        return (3, 8, 8), [(3, None, True), (13, None, False), (6, None, True), (-1, None, False), (12, None, True), (1 << 40, None, False),
                           (0, None, True)]
    if kind == "crop":
        Hs, th = 20, 16
        return (3, 20, 20, 16, 16), [(3, [1, 2, 1], True), (13, [0, 0, 0], False), (6, [4, 4, 0], True), (-1, [0, 0, 0], False),
                                     (5, [Hs - th + 1, 0, 0], False), (2, [2, 2, 2], False), (12, [0, 3, 1], True), (7, [0, -1, 0], False),
                                     (1, [-1, 0, 1], False)]
    return (2, 20, 26, 2, 3), [(3, [1, 2, 10, 9, 1], True), (13, [0, 0, 4, 4, 0], False), (6, [4, 4, 16, 20, 0], True),
                               (-1, [0, 0, 4, 4, 0], False), (5, [-1, 0, 4, 4, 0], False), (2, [0, -1, 4, 4, 1], False),
                               (12, [0, 3, 5, 7, 1], True), (7, [17, 0, 4, 4, 0], False), (1, [0, 23, 4, 4, 0], False),
                               (4, [2, 2, 0, 4, 0], False), (4, [2, 2, 4, 0, 1], False), (0, [2, 2, 2, 2, 0], True),
                               (8, [2, 2, 4, 4, 2], False), (9, [0, 0, 17, 4, 0], False), (10, [0, 0, 4, 25, 1], False),
                               (11, [19, 25, 1, 1, 1], True), (3, [0, 0, 4, 4, -1], False)]


@pytest.mark.parametrize("kind", ["plain", "crop", "resized"])
def test_bad_rows_copy_nothing_and_get_label_minus_one(kind):
    """Defined behaviour for tables the host would never upload, between good rows: the bad row keeps its prefill and gets label
    -1, every other row is bitwise the fp32 entry's on the decoded frames."""
    geo, rows = _bad_rows(kind)
    t = _tasks(3, *geo[:3])
    idx = torch.tensor([r[0] for r in rows])
    params = None if kind == "plain" else torch.tensor([r[1] for r in rows], dtype=torch.int32)
    good = [k for k, r in enumerate(rows) if r[2]]
    bad = [k for k, r in enumerate(rows) if not r[2]]
    row_shape = (geo[0] * geo[1] * geo[2],) if kind == "plain" else (geo[0], geo[3], geo[4])
    x = torch.full((len(rows),) + row_shape, -7.0, device=DEV)
    labels = torch.full((len(rows),), 99, dtype=torch.int64, device=DEV)
    _launch_pair(kind, t, geo, idx, params, x_out=x, labels_out=labels)
    _, want = _launch_pair(kind, t, geo, idx[good], None if params is None else params[good])
    assert bool((x[bad] == -7.0).all()) and labels[bad].tolist() == [-1] * len(bad)
    assert torch.equal(_bits(x[good]), _bits(want[0])) and torch.equal(labels[good], want[1])
    assert torch.equal(labels[good].cpu(), t["labels"][idx[good]])


def test_ops_conventions():
    """CPU tensors are refused, a table of mixed dtypes is refused, B = 0 gives empty outputs, a wrong table shape asserts."""
    from clsurvey_amd import ops
    geo = (3, 10, 12, 8, 8)
    t = _tasks(3, 3, 10, 12)
    tb, _ = _tables(t)
    idx = torch.tensor([0, 1], device=DEV)
    p3 = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    p5 = torch.tensor([[0, 0, 4, 4, 0]] * 2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.gather_tasks_u8(tb, 3, 120, t["lut"].cpu(), idx)
    with pytest.raises(RuntimeError):
        ops.gather_tasks_crop_flip_u8(tb, geo, t["lut"], idx, p3.cpu())
    with pytest.raises(RuntimeError):
        ops.gather_tasks_resized_crop_flip_u8(tb, geo, t["lut"], idx.cpu(), p5)
    with pytest.raises(AssertionError):
        ops.gather_tasks_crop_flip_u8(tb, geo, t["lut"][:2].contiguous(), idx, p3)
    with pytest.raises(AssertionError):
        ops.gather_tasks_resized_crop_flip_u8(tb, geo, t["lut"], idx, p3)
    with pytest.raises(AssertionError):
        ops.task_table([t["bx"][0], t["fs"][1]], t["ys"][:2], t["cum"][:2], t["shifts"][:2], DEV)
    x0, y0 = ops.gather_tasks_u8(tb, 3, 120, t["lut"], idx[:0])
    assert tuple(x0.shape) == (0, 360) and tuple(y0.shape) == (0,)
    x0, y0 = ops.gather_tasks_crop_flip_u8(tb, geo, t["lut"], idx[:0], p3[:0])
    assert tuple(x0.shape) == (0, 3, 8, 8) and tuple(y0.shape) == (0,)
    x0, y0 = ops.gather_tasks_resized_crop_flip_u8(tb, geo, t["lut"], idx[:0], p5[:0])
    assert tuple(x0.shape) == (0, 3, 8, 8) and tuple(y0.shape) == (0,)


# ---------------------------------------------------------------------------------------------- loaders
def _byte_tasks(n_tasks, transform, n=24, hw=20, seed=31):
    from clsurvey_amd.data import ByteTaskDataset
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_tasks):
        x = torch.randint(0, 256, (n, 3, hw, hw), generator=gen, dtype=torch.uint8)
        y = torch.randint(0, 4, (n,), generator=gen)
        out.append(ByteTaskDataset(x.to(DEV), y.to(DEV), [str(k) for k in range(4)], MEAN, STD, transform=transform))
    return out


def _transform(name):
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip
    if name == "none":
        return None
    if name == "crop":
        return RandomCropFlip((16, 16))
    ext = torch.tensor([[20 - (k % 3), 17 + (k % 4)] for k in range(24)]) if name == "resized_extents" else None
    return RandomResizedCropFlip((16, 16), extents=ext)


def _epoch(loader):
    torch.manual_seed(3)
    random.seed(3)
    np.random.seed(3)
    batches = [(x.clone(), y.clone(), None if loader.last_idx is None else loader.last_idx.clone(),
                None if loader.last_idx_host is None else loader.last_idx_host.clone()) for x, y in loader]
    return batches, (torch.get_rng_state(), random.getstate(), np.random.get_state()[1].tolist())


def _same_epochs(byte_loader, float_loader, frames, out_shape):
    assert tuple(byte_loader.x.shape) == (0,) + out_shape and byte_loader.x.dtype == torch.float32
    assert tuple(float_loader.x.shape[1:]) == out_shape and len(byte_loader) == len(float_loader)
    got, state_b = _epoch(byte_loader)
    want, state_f = _epoch(float_loader)
    assert torch.equal(state_b[0], state_f[0]) and state_b[1] == state_f[1] and state_b[2] == state_f[2]
    assert len(got) == len(want) == len(byte_loader)
    for (xb, yb, ib, hb), (xf, yf, jf, _) in zip(got, want):
        assert xb.dtype == torch.float32 and tuple(xb.shape[1:]) == out_shape
        assert torch.equal(_bits(xb), _bits(xf)) and torch.equal(yb, yf)
        assert torch.equal(ib.cpu(), hb) and ib.dtype == torch.int64
        if jf is not None:
            assert torch.equal(ib, jf)
        else:                                                     # a plain float loader keeps no sample numbers: the rows say them
            assert torch.equal(_bits(xb), _bits(frames[ib]))
    return got


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "in_order"])
@pytest.mark.parametrize("name", ["none", "crop", "resized", "resized_extents"])
def test_device_loader_serves_the_decoded_loaders_epoch(name, shuffle):
    from clsurvey_amd.data import DeviceLoader
    task = _byte_tasks(1, _transform(name))[0]
    dec = task.decoded()
    assert task.x.dtype == torch.uint8 and dec.x.dtype == torch.float32 and dec.transform is task.transform
    loader = DeviceLoader(task, 7, shuffle, DEV)
    assert loader.transform is task.transform and loader.frames[0].dtype == torch.uint8
    got = _same_epochs(loader, DeviceLoader(dec, 7, shuffle, DEV), dec.x, (3, 20, 20) if name == "none" else (3, 16, 16))
    assert [b[0].shape[0] for b in got] == [7, 7, 7, 3]
    if not shuffle:
        assert torch.equal(torch.cat([b[3] for b in got]), torch.arange(24))
    lut = loader._lut
    list(loader)
    assert loader._lut is lut                                      # uploaded once per loader


@pytest.mark.parametrize("name", ["none", "crop", "resized"])
def test_multi_task_loader_serves_the_decoded_loaders_epoch(name):
    from clsurvey_amd.data import MultiTaskLoader, TaskList
    tasks = _byte_tasks(3, _transform(name))
    dec = [t.decoded() for t in tasks]
    loader = MultiTaskLoader(TaskList(tasks), 7, True, DEV)
    assert len(loader.frames) == 3 and all(f.dtype == torch.uint8 and f.data_ptr() == t.x.data_ptr() for f, t in zip(loader.frames, tasks))
    got = _same_epochs(loader, MultiTaskLoader(TaskList(dec), 7, True, DEV), torch.cat([d.x for d in dec]),
                       (3, 20, 20) if name == "none" else (3, 16, 16))
    assert sorted(torch.cat([b[3] for b in got]).tolist()) == list(range(72))
    assert int(torch.cat([b[1] for b in got]).max()) >= 8          # labels of the third task are shifted


# ---------------------------------------------------------------------------------------------- trainers
def _seeds(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _synthetic_byte_dict(root, **kw):
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=1, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="u8", u8_frames=True, **kw)
    return load_task_datasets(ds.get_task_dataset_path("1", rnd_transform=bool(kw)), DEV)


def test_finetune_on_a_byte_dict_is_the_run_on_its_decoded_dict(tmp_path):
    from clsurvey_amd import models
    from clsurvey_amd.data import ByteTaskDataset, DeviceLoader
    from clsurvey_amd.methods import finetune
    root = str(tmp_path)
    dsets = _synthetic_byte_dict(root)
    assert all(isinstance(d, ByteTaskDataset) and d.x.is_cuda and d.x.element_size() == 1 for d in dsets.values())
    torch.manual_seed(0)
    base = os.path.join(root, "base.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), base)
    params, accs = [], []
    for tag in ("bytes", "decoded"):
        per = {s: dsets[s] if tag == "bytes" else dsets[s].decoded() for s in ("train", "val")}
        _seeds(7)
        loaders = {s: DeviceLoader(per[s], 40, True, DEV) for s in per}
        assert tuple(loaders["train"].x.shape[1:]) == (3, 32, 32)
        model, acc = finetune.fine_tune_SGD(loaders, {s: len(per[s]) for s in per}, {s: [per[s].classes] for s in per},
                                            model_path=base, exp_dir=os.path.join(root, tag), num_epochs=2, lr=1e-2, device=DEV,
                                            batch_size=40)
        params.append([p.detach().clone() for p in model.parameters()])
        accs.append(acc)
    start = list(torch.load(base, weights_only=False).parameters())
    assert any(not torch.equal(a.cpu(), s) for a, s in zip(params[0], start))        # the epochs did train
    for a, b in zip(*params):
        assert torch.equal(_bits(a), _bits(b))
    assert float(accs[0]) == float(accs[1])


def _rehearsal_args(root, tag, dsets):
    from clsurvey_amd import models
    torch.manual_seed(0)
    prev = os.path.join(root, "prev.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), prev)
    return dict(task_name="1", task_count=1, prev_model_path=prev, n_outputs=8, method="baseline_rehearsal_partial_mem", n_memories=6,
                n_tasks=2, dataset_path=dsets, postprocess=False, is_scratch_model=True, save_path=os.path.join(root, tag),
                n_epochs=1, batch_size=16, lr=1e-2)


def test_rehearsal_partial_mem_on_byte_splits_stores_the_crops_it_was_served(tmp_path):
    """Crop mode (no transform): the store holds fp32 rows, those of the run on the decoded splits.  A byte train split with a
    transform is refused before any loader is built."""
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dsets = _synthetic_byte_dict(root)
    runs = []
    for tag in ("bytes", "decoded"):
        per = dsets if tag == "bytes" else {s: d.decoded() for s, d in dsets.items()}
        _seeds(11)
        model, acc = gem_main.main(_rehearsal_args(root, tag, per), [4, 4], device=DEV)
        runs.append((model, acc))
    a, b = runs[0][0], runs[1][0]
    assert a.exemplar_transform is None and a.store_x.dtype == torch.float32 and tuple(a.store_x.shape[1:]) == (3, 32, 32)
    assert float(a.store_x[:6].abs().sum(dim=(1, 2, 3)).min()) > 0
    assert torch.equal(_bits(a.store_x), _bits(b.store_x)) and torch.equal(a.store_y, b.store_y)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(_bits(p.detach()), _bits(q.detach()))
    assert runs[0][1] == runs[1][1]
    augmented = _synthetic_byte_dict(os.path.join(root, "aug"), rnd_margin=4)
    assert augmented["train"].transform is not None and augmented["train"].x.dtype == torch.uint8
    with pytest.raises(NotImplementedError, match="byte frames"):
        gem_main.main(_rehearsal_args(root, "aug_run", augmented), [4, 4], device=DEV)


def test_icarl_herding_on_a_byte_split_ranks_as_on_the_decoded_split():
    import g37_common as I
    from clsurvey_amd.data import ByteTaskDataset
    from clsurvey_amd.methods.icarl import IcarlNet
    x, y = I.task_data(0)
    xb = (torch.from_numpy(x) * 48 + 128).round().clamp(0, 255).to(torch.uint8)
    byte = ByteTaskDataset(xb.to(DEV), torch.from_numpy(y).to(DEV), [], [128.0 / 255] * 3, [48.0 / 255] * 3)
    res = []
    for split in (byte, byte.decoded()):
        torch.manual_seed(1)
        w = IcarlNet(I.make_net(), I.N_OUT, I.N_TASKS, I.NC_PER_TASK, I.N_MEMORIES, I.LR, I.WD, I.REG, I.B + I.N_APPEND, (3, I.HW, I.HW), "cuda")
        w.manage_memory(0, types.SimpleNamespace(task_imgfolders={"train": split}, batch_size=I.HERD_BATCH))
        res.append((w.last_ranking[0].clone(), list(w.last_ranking[1]), w.store_x.clone(), list(w.class_len)))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and res[0][3] == res[1][3] and sum(res[0][3]) > 0
    assert res[0][2].dtype == torch.float32 and torch.equal(_bits(res[0][2]), _bits(res[1][2])) and float(res[0][2].abs().sum()) > 0


# ---------------------------------------------------------------------------------------------- through the driver
def test_ewc_through_the_driver_on_byte_tasks_with_a_margin(tmp_path):
    from clsurvey_amd import data, models
    from clsurvey_amd.framework import driver
    root = str(tmp_path)
    torch.manual_seed(0)
    m = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(m, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))
    common = ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "3", "--batch_size", "40", "--saving_freq", "100",
              "--results_root", root, "--synthetic", "2,4,160,40,40,32", "--u8_frames", "--rnd_margin", "4"]
    driver.main(common + ["--method_name", "SI", "--runmode", "first_task_basemodel_dump"])
    out = driver.main(common + ["--method_name", "EWC", "--test", "--drop_margin", "0.05"])
    res = out["results"]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("EWC on byte tasks:", accs)
    assert sorted(res) == [0, 1] and len(accs) == 3 and all(a == a and 0.0 <= a <= 100.0 for a in accs)
    tdir = os.path.join(out["manager"].parent_exp_dir, "task_2", "TASK_TRAINING")
    assert os.path.exists(os.path.join(tdir, "SUCCESS.FLAG")) and os.path.exists(os.path.join(tdir, "best_model.pth.tar"))
    folder = os.path.join(root, "data", "synthetic_tiny_imagenet")
    files = sorted(f for f in os.listdir(folder) if f.endswith(".pth.tar"))
    assert files == ["task_1_rndtrans.pth.tar", "task_2_rndtrans.pth.tar"]
    # the cache accounting: what the files' tensors really take
    data._TASK_CACHE.clear()
    data._TASK_CACHE_BYTES[0] = 0
    real = 0
    for f in files:
        on_disk = torch.load(os.path.join(folder, f), weights_only=False)
        assert all(isinstance(d, data.ByteTaskDataset) and d.x.element_size() == 1 for d in on_disk.values())
        assert tuple(on_disk["train"].x.shape[1:]) == (3, 36, 36) and on_disk["train"].transform is not None
        real += sum(d.x.numel() + 8 * d.y.numel() for d in on_disk.values())
        loaded = data.load_task_datasets(os.path.join(folder, f), DEV)
        assert all(isinstance(d, data.ByteTaskDataset) and d.x.is_cuda and d.x.element_size() == 1 for d in loaded.values())
    assert data._TASK_CACHE_BYTES[0] == real
