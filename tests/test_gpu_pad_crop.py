"""Padded RandomCrop + flip on the GPU: clhip_gather_tasks_pad_crop_flip against the index-map restatement of
tests/pad_crop_ref.py (a copy: bitwise, no tolerance) in all four modes, per-sample extents, its safety rule, the byte entry
against the fp32 entry on the decoded frames, the loaders against (order, draw_pad_crop_flip(base seed)) recomputed on the host,
a spec without freedom as the identity of a training epoch, and `--rnd_pad` through the driver."""
import functools
import os
import sys
from itertools import accumulate

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pad_crop_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # distinct per channel
FILL = [0.25, -1.5, 3.0]                                          # distinct per channel, none a value randn gives
FILL_BYTES = [3, 200, 128]
IDX = {3: [0, 4, 5, 6, 12, 4, 9, 5, 11], 1: [0, 4, 5, 6, 12, 4, 9, 5, 11]}     # T = 3: across every task boundary; sample 4 twice


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sizes(T):
    return ([5, 1, 7], [3, 2, 4]) if T == 3 else ([13], [9])


@functools.lru_cache(maxsize=None)
def _tasks(T, C, Hs, Ws):
    """T = 3 tasks of 5 / 1 / 7 frames or one of 13, floats on the CPU; made once per shape."""
    gen = torch.Generator().manual_seed(1000 * T + Hs + 3 * Ws)
    sizes, ncls = _sizes(T)
    xs = [torch.randn((n, C, Hs, Ws), generator=gen) for n in sizes]
    ys = [torch.randint(0, k, (n,), generator=gen) for n, k in zip(sizes, ncls)]
    shifts = [0] + list(accumulate(ncls))[:-1]
    return xs, ys, list(accumulate(sizes)), shifts, torch.cat([y + s for y, s in zip(ys, shifts)])


def _table(xs, ys, cum, shifts):
    from clsurvey_amd import ops
    dev_x, dev_y = [x.to(DEV) for x in xs], [y.to(DEV) for y in ys]
    return ops.task_table(dev_x, dev_y, cum, shifts, DEV), (dev_x, dev_y)          # (the table holds pointers: keep the tensors)


def _fill(C=3):
    return torch.tensor(FILL[:C], device=DEV)


@functools.lru_cache(maxsize=None)
def _reference(T, geometry, mode, pads):
    """(idx, params, restatement) of the 9 corner rows on full extents; computed once, shared by the tests below."""
    Hs, Ws, th, tw, _ = geometry
    xs = _tasks(T, 3, Hs, Ws)[0]
    idx = torch.tensor(IDX[T])
    params = ref.corner_rows(Hs, Ws, th, tw, pads)
    return idx, params, ref.restate(torch.cat(xs), idx, params, th, tw, mode, FILL)


CASES = ref.cases()
CASE_ARGS = dict(argnames="geometry,mode,pads", argvalues=[c[1:] for c in CASES], ids=[c[0] for c in CASES])


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize(**CASE_ARGS)
def test_kernel_is_bitwise_pad_crop_then_flip(geometry, mode, pads):
    """T in {1, 3} and B in {1, 9}: top and left at both ends of their ranges, strictly inside the image, odd offsets, mixed
    flips, one sample under two parameter rows."""
    from clsurvey_amd import ops
    Hs, Ws, th, tw, _ = geometry
    for T in (3, 1):
        xs, ys, cum, shifts, labels = _tasks(T, 3, Hs, Ws)
        table, keep = _table(xs, ys, cum, shifts)
        idx, params, want = _reference(T, geometry, mode, pads)
        for rows in (slice(0, 9), slice(1, 2)):                                     # B = 9, B = 1 (the far corner, flipped)
            x, y = ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), mode, pads, _fill(), idx[rows].to(DEV),
                                                  params[rows].to(DEV).contiguous())
            assert tuple(x.shape) == (len(idx[rows]), 3, th, tw) and x.dtype == torch.float32
            assert torch.equal(_bits(x.cpu()), _bits(want[rows]))
            assert torch.equal(y.cpu(), labels[idx[rows]])
    assert not torch.isnan(want).any()


def test_the_reference_rows_touch_every_border_and_the_interior():
    """What the geometries were chosen for, asserted on the parameter rows themselves (no device needed, but it belongs here)."""
    from clsurvey_amd import _lib
    for _, (Hs, Ws, th, tw, _), mode, pads in CASES:
        p = ref.corner_rows(Hs, Ws, th, tw, pads)
        pl, pt, pr, pb = pads
        assert int(p[:, 0].min()) == -pt and int(p[:, 0].max()) == Hs + pb - th
        assert int(p[:, 1].min()) == -pl and int(p[:, 1].max()) == Ws + pr - tw
        assert sorted(set(p[:, 2].tolist())) == [0, 1]
        if Hs >= th and Ws >= tw:                                                   # a row that touches no border
            assert any(0 <= t and t + th <= Hs and 0 <= l and l + tw <= Ws for t, l, *_ in p.tolist())
    rpb = _lib.lib().clhip_crop_rows_per_block
    assert rpb(64) == 64 and -(-70 // rpb(64)) == 2 and 70 % rpb(64) == 6           # two chunks of lines, a short last one
    assert rpb(4100) == 1 and 4100 > 4096                                          # a line longer than a block's segment
    assert any(l % 2 for _, l, *_ in ref.corner_rows(20, 20, 16, 16, (4, 4, 4, 4)).tolist())   # vector stores, odd left


EXTENT_GEOMETRIES = [(13, 11, 8, 7, (2, 2, 2, 2)), (20, 20, 16, 16, (4, 4, 4, 4)), (12, 12, 8, 8, (1, 2, 3, 0))]


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("geometry", EXTENT_GEOMETRIES, ids=["%dx%d_to_%dx%d" % g[:4] for g in EXTENT_GEOMETRIES])
def test_the_maps_use_each_samples_own_extent(geometry, mode):
    """Frames stored top-left anchored in Hs x Ws, NaN outside each sample's extent, mixed extents: the output is the restatement
    on the valid part and holds no NaN, so nothing outside an extent was read."""
    from clsurvey_amd import ops
    Hs, Ws, th, tw, pads = geometry
    xs, ys, cum, shifts, labels = _tasks(3, 3, Hs, Ws)
    ext = [(Hs - (g % 4), Ws - (g % 3)) for g in range(13)]                       # per sample; (Hs, Ws) among them
    frames = torch.cat(xs).clone()
    for g, (h, w) in enumerate(ext):
        frames[g, :, h:, :] = float("nan")
        frames[g, :, :, w:] = float("nan")
    assert torch.isnan(frames).any()
    idx = torch.tensor(IDX[3])
    params = torch.stack([ref.corner_rows(*ext[g], th, tw, pads)[k] for k, g in enumerate(idx.tolist())])
    assert len(set(map(tuple, params[:, 3:].tolist()))) > 3
    split = [frames[a:b] for a, b in zip([0] + cum[:-1], cum)]
    table, keep = _table(split, ys, cum, shifts)
    x, y = ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), mode, pads, _fill(), idx.to(DEV), params.to(DEV))
    want = ref.restate(frames, idx, params, th, tw, mode, FILL)
    assert not torch.isnan(want).any() and not torch.isnan(x).any()
    assert torch.equal(_bits(x.cpu()), _bits(want)) and torch.equal(y.cpu(), labels[idx])


@pytest.mark.parametrize("mode", ref.MODES)
def test_zero_pads_are_the_plain_crop(mode):
    from clsurvey_amd import ops
    Hs, Ws, th, tw = 20, 20, 16, 16
    xs, ys, cum, shifts, _ = _tasks(3, 3, Hs, Ws)
    table, keep = _table(xs, ys, cum, shifts)
    idx = torch.tensor(IDX[3]).to(DEV)
    p3 = ref.corner_rows(Hs, Ws, th, tw, (0, 0, 0, 0))[:, :3].contiguous()
    assert int(p3[:, :2].min()) == 0 and int(p3[:, :2].max()) == 4
    p5 = torch.cat([p3, torch.tensor([[Hs, Ws]] * 9, dtype=torch.int32)], 1)
    a = ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), mode, (0, 0, 0, 0), _fill(), idx, p5.to(DEV))
    b = ops.gather_tasks_crop_flip(table, (3, Hs, Ws, th, tw), idx, p3.to(DEV))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode", ref.MODES)
def test_unaligned_output_takes_the_plain_path(mode):
    """tw % 4 == 0 but x_out 4 bytes off a 16-byte boundary: no vector stores, same bytes, the guard element untouched."""
    from clsurvey_amd import ops
    geometry = ref.GEOMETRIES[1]
    Hs, Ws, th, tw, pads = geometry
    xs, ys, cum, shifts, _ = _tasks(3, 3, Hs, Ws)
    table, keep = _table(xs, ys, cum, shifts)
    idx, params, want = _reference(3, geometry, mode, pads)
    buf = torch.full((1 + 9 * 3 * th * tw,), -7.0, device=DEV)
    assert buf[1:].data_ptr() % 16 == 4
    x, _ = ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), mode, pads, _fill(), idx.to(DEV), params.to(DEV), x_out=buf[1:])
    assert x.data_ptr() == buf[1:].data_ptr()
    assert torch.equal(_bits(x.cpu().view(9, 3, th, tw)), _bits(want)) and float(buf[0]) == -7.0


def test_two_launches_are_bitwise_equal():
    from clsurvey_amd import ops
    geometry = ref.GEOMETRIES[6]                                                    # two chunks of lines
    Hs, Ws, th, tw, pads = geometry
    xs, ys, cum, shifts, _ = _tasks(3, 3, Hs, Ws)
    table, keep = _table(xs, ys, cum, shifts)
    idx, params, _ = _reference(3, geometry, "symmetric", pads)
    a = ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), "symmetric", pads, _fill(), idx.to(DEV), params.to(DEV))
    b = ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), "symmetric", pads, _fill(), idx.to(DEV), params.to(DEV))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode", ref.MODES)
def test_bad_rows_copy_nothing_and_get_label_minus_one(mode):
    """The kernel's defined behaviour for a table the host would never upload, between good rows.  Pads (pl, pt, pr, pb) =
    (3, 4, 2, 1) on 12 x 12 frames cropped to 8 x 8: top in [-4, h - 7], left in [-3, w - 6].  Row 14 has an extent of 4 lines:
    its top is in range, but reflect takes pads up to 3 there — bad under reflect, good under the other modes."""
    from clsurvey_amd import ops
    Hs, Ws, th, tw, pads = 12, 12, 8, 8, (3, 4, 2, 1)
    pl, pt, pr, pb = pads
    xs, ys, cum, shifts, labels = _tasks(3, 3, Hs, Ws)
    table, keep = _table(xs, ys, cum, shifts)
    rows = [(3, [1, 2, 1, 12, 12], True),
            (13, [0, 0, 0, 12, 12], False),                                          # sample number = total
            (6, [-pt, Ws + pr - tw, 0, 12, 12], True),
            (-1, [0, 0, 0, 12, 12], False),                                          # sample number -1
            (5, [-pt - 1, 0, 0, 12, 12], False),                                     # top one before its range
            (2, [Hs + pb - th + 1, 0, 1, 12, 12], False),                            # top one past it
            (12, [Hs + pb - th, -pl, 1, 12, 12], True),
            (7, [0, -pl - 1, 0, 12, 12], False),                                     # left one before its range
            (1, [0, Ws + pr - tw + 1, 1, 12, 12], False),                            # left one past it
            (4, [0, 0, 0, 0, 12], False),                                            # h = 0
            (0, [0, 0, 0, Hs + 1, 12], False),                                       # h = Hs + 1
            (9, [0, 0, 2, 12, 12], False),                                           # flip = 2
            (8, [0, 0, 0, 12, Ws + 1], False),                                       # w = Ws + 1
            (10, [0, 0, 1, 12, 0], False),                                           # w = 0
            (11, [-pt, 1, 1, 4, 12], mode != "reflect"),                             # extent too small for reflect's pads
            (2, [10 + pb - th, 9 + pr - tw, 1, 10, 9], True),                        # a smaller extent, its own far corner
            (5, [10 + pb - th + 1, 0, 0, 10, 9], False)]                             # in range for the frame, not for the extent
    idx = torch.tensor([r[0] for r in rows])
    params = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    good = [k for k, r in enumerate(rows) if r[2]]
    bad = [k for k, r in enumerate(rows) if not r[2]]
    assert len(bad) == (13 if mode == "reflect" else 12)
    x = torch.full((len(rows), 3, th, tw), -7.0, device=DEV)
    lab = torch.full((len(rows),), 99, dtype=torch.int64, device=DEV)
    ops.gather_tasks_pad_crop_flip(table, (3, Hs, Ws, th, tw), mode, pads, _fill(), idx.to(DEV), params.to(DEV), x_out=x, labels_out=lab)
    x, lab = x.cpu(), lab.cpu()
    assert bool((x[bad] == -7.0).all()) and lab[bad].tolist() == [-1] * len(bad)
    want = ref.restate(torch.cat(xs), idx[good], params[good], th, tw, mode, FILL)
    assert torch.equal(_bits(x[good]), _bits(want)) and torch.equal(lab[good], labels[idx[good]])


# ---------------------------------------------------------------------------------------------- byte frames
def _lut():
    from clsurvey_amd.data import norm_lut
    return norm_lut(torch.tensor(MEAN), torch.tensor(STD))


@functools.lru_cache(maxsize=None)
def _byte_tasks(T, Hs, Ws, odd_base):
    """Byte frames and their decoded twins on the device; odd_base: every frame tensor starts one byte into its storage."""
    gen = torch.Generator().manual_seed(500 * T + Hs + Ws)
    sizes, ncls = _sizes(T)
    xs = [torch.randint(0, 256, (n, 3, Hs, Ws), generator=gen, dtype=torch.uint8) for n in sizes]
    ys = [torch.randint(0, k, (n,), generator=gen).to(DEV) for n, k in zip(sizes, ncls)]
    lut = _lut()
    fs = [torch.stack([lut[c][x[:, c].long()] for c in range(3)], 1).to(DEV) for x in xs]
    if odd_base:
        bufs = [torch.empty((x.numel() + 1,), dtype=torch.uint8, device=DEV) for x in xs]
        bx = [b[1:].view(x.shape).copy_(x) for b, x in zip(bufs, xs)]
        assert all(v.data_ptr() % 2 == 1 and v.is_contiguous() for v in bx)
    else:
        bx = [x.to(DEV) for x in xs]
    return bx, fs, ys, list(accumulate(sizes)), [0] + list(accumulate(ncls))[:-1]


@pytest.mark.parametrize(**CASE_ARGS)
def test_byte_entry_is_the_fp32_entry_on_the_decoded_frames(geometry, mode, pads):
    """fill = lut[c, fill byte of c]; T = 3 on aligned frames, T = 1 on frames that start at an odd address."""
    from clsurvey_amd import ops
    Hs, Ws, th, tw, _ = geometry
    lut = _lut()
    fill = torch.stack([lut[c, v] for c, v in enumerate(FILL_BYTES)]).to(DEV)
    for T, odd in ((3, False), (1, True)):
        bx, fs, ys, cum, shifts = _byte_tasks(T, Hs, Ws, odd)
        tb, tf = ops.task_table(bx, ys, cum, shifts, DEV), ops.task_table(fs, ys, cum, shifts, DEV)
        idx = torch.tensor(IDX[T]).to(DEV)
        params = ref.corner_rows(Hs, Ws, th, tw, pads).to(DEV)
        got = ops.gather_tasks_pad_crop_flip_u8(tb, (3, Hs, Ws, th, tw), mode, pads, fill, lut.to(DEV), idx, params)
        want = ops.gather_tasks_pad_crop_flip(tf, (3, Hs, Ws, th, tw), mode, pads, fill, idx, params)
        assert got[0].dtype == torch.float32 and got[0].shape == want[0].shape
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(got[1], want[1])
    if mode == "constant" and pads[0]:                                              # and the fill did come out of the table
        assert bool((got[0][0, 1, 0, :pads[0]] == float(lut[1, 200])).all())


# ---------------------------------------------------------------------------------------------- loaders
def _sequence(root, **kw):
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(24, 8, 8), hw=16, noise=0.4,
                               name="pad2", rnd_pad=4, **kw)
    return ds, [ds.get_task_dataset_path(str(t), rnd_transform=True) for t in (1, 2)]


def _host_epoch(n, shuffle, spec, frame_hw):
    """What an augmented loader does with the global generator and its base seed, restated: (order, parameter table)."""
    from clsurvey_amd.data import draw_pad_crop_flip
    base = int(torch.empty((), dtype=torch.int64).random_().item())
    perm = None
    if shuffle:
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    table = draw_pad_crop_flip(n, spec, frame_hw, torch.Generator().manual_seed(base), order=perm)
    return (torch.arange(n) if perm is None else perm), table


@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "in_order"])
@pytest.mark.parametrize("u8", [False, True], ids=["float", "u8_frames"])
@pytest.mark.parametrize("multi", [False, True], ids=["DeviceLoader", "MultiTaskLoader"])
def test_loader_serves_the_restatement_of_its_own_draws(tmp_path, multi, u8, shuffle):
    from clsurvey_amd.data import ByteTaskDataset, DeviceLoader, MultiTaskLoader, RandomPadCropFlip, TaskList, load_task_datasets
    mode = "reflect" if shuffle else "constant"
    ds, paths = _sequence(str(tmp_path), pad_mode=mode, u8_frames=u8)
    tasks = [load_task_datasets(p, DEV)["train"] for p in paths]
    assert all(isinstance(t.transform, RandomPadCropFlip) and t.x.is_cuda and tuple(t.x.shape) == (24, 3, 16, 16) for t in tasks)
    assert all(isinstance(t, ByteTaskDataset) == u8 for t in tasks)
    used = tasks if multi else tasks[:1]
    loader = MultiTaskLoader(TaskList(used), 7, shuffle, DEV) if multi else DeviceLoader(used[0], 7, shuffle, DEV)
    plain = [load_task_datasets(ds.get_task_dataset_path(str(t)), DEV)["train"] for t in (1, 2)][:len(used)]
    plain_loader = MultiTaskLoader(TaskList(plain), 7, shuffle, DEV) if multi else DeviceLoader(plain[0], 7, shuffle, DEV)
    frames = torch.cat([(t.decoded() if u8 else t).x for t in used]).cpu()
    labels = torch.cat([t.y + s for t, s in zip(used, (0, 4))]).cpu()
    fill = [0.0, 0.0, 0.0]                                                          # 0.0, or byte 128 = exactly 0.0
    n = frames.shape[0]
    assert tuple(loader.x.shape) == (0, 3, 16, 16) and len(loader) == (n + 6) // 7 and loader.frames[0].data_ptr() == used[0].x.data_ptr()
    torch.manual_seed(3)
    got = list(loader)
    after = torch.get_rng_state()
    torch.manual_seed(3)
    list(plain_loader)
    assert torch.equal(after, torch.get_rng_state())                                # the global generator: as the plain loader's
    torch.manual_seed(3)
    order, table = _host_epoch(n, shuffle, loader.transform, (16, 16))
    assert torch.equal(after, torch.get_rng_state())
    assert [b[0].shape[0] for b in got] == [7] * (n // 7) + ([n % 7] if n % 7 else [])
    want = ref.restate(frames, order, table, 16, 16, mode, fill)
    assert torch.equal(_bits(torch.cat([b[0] for b in got]).cpu()), _bits(want))
    assert torch.equal(torch.cat([b[1] for b in got]).cpu(), labels[order])
    assert len(set(map(tuple, table.tolist()))) > 5 and int(table[:, 0].min()) < 0 and int(table[:, 1].max()) > 0
    fill_dev = loader._fill
    assert fill_dev.tolist() == fill
    second = list(loader)
    assert loader._fill is fill_dev                                                 # uploaded once per loader
    if not shuffle:
        a, b = torch.cat([v[0] for v in got]), torch.cat([v[0] for v in second])
        assert torch.equal(torch.cat([v[1] for v in second]).cpu(), labels) and not torch.equal(a, b)


@pytest.mark.parametrize("mode", ["constant", "symmetric"])
@pytest.mark.parametrize("multi", [False, True], ids=["DeviceLoader", "MultiTaskLoader"])
def test_byte_loaders_serve_the_decoded_loaders_epoch(multi, mode):
    """Per-channel fill bytes and mean / std that differ per channel, per-sample extents: batches, labels, last_idx and the
    global generator are those of the loader over .decoded()."""
    from clsurvey_amd.data import ByteTaskDataset, DeviceLoader, MultiTaskLoader, RandomPadCropFlip, TaskList
    gen = torch.Generator().manual_seed(31)
    ext = torch.tensor([[20 - (k % 3), 17 + (k % 4)] for k in range(24)])
    spec = RandomPadCropFlip((16, 16), (3, 4, 2, 1), fill=tuple(FILL_BYTES), padding_mode=mode, extents=ext)
    tasks = []
    for _ in range(3 if multi else 1):
        x = torch.randint(0, 256, (24, 3, 20, 20), generator=gen, dtype=torch.uint8)
        y = torch.randint(0, 4, (24,), generator=gen)
        tasks.append(ByteTaskDataset(x.to(DEV), y.to(DEV), [str(k) for k in range(4)], MEAN, STD, transform=spec))
    dec = [t.decoded() for t in tasks]
    lut = _lut()
    assert torch.equal(torch.tensor(dec[0].transform.fill, dtype=torch.float32), torch.stack([lut[c, v] for c, v in enumerate(FILL_BYTES)]))
    if multi:
        a, b = MultiTaskLoader(TaskList(tasks), 7, True, DEV), MultiTaskLoader(TaskList(dec), 7, True, DEV)
    else:
        a, b = DeviceLoader(tasks[0], 7, True, DEV), DeviceLoader(dec[0], 7, True, DEV)
    assert a.frames[0].dtype == torch.uint8 and b.frames[0].dtype == torch.float32 and tuple(a.x.shape) == (0, 3, 16, 16)
    epochs = []
    for loader in (a, b):
        torch.manual_seed(3)
        rows = [(x.clone(), y.clone(), loader.last_idx.clone(), loader.last_idx_host.clone()) for x, y in loader]
        epochs.append((rows, torch.get_rng_state()))
    assert torch.equal(epochs[0][1], epochs[1][1]) and len(epochs[0][0]) == len(epochs[1][0]) == len(a)
    for (xb, yb, ib, hb), (xf, yf, jf, hf) in zip(*[e[0] for e in epochs]):
        assert torch.equal(_bits(xb), _bits(xf)) and torch.equal(yb, yf) and torch.equal(ib, jf) and torch.equal(hb, hf)
        assert torch.equal(ib.cpu(), hb) and not torch.isnan(xb).any()
    assert torch.equal(_bits(a._fill), _bits(b._fill))


# ---------------------------------------------------------------------------------------------- trainers
def test_spec_without_freedom_is_the_identity_of_a_training_epoch(tmp_path):
    """Pads 0, size == frame and p = 0: the padded path changes nothing but the pixels, and here not those — one epoch of
    fine_tune_SGD leaves the parameters bitwise equal to the same epoch through the plain loader."""
    from clsurvey_amd import models
    from clsurvey_amd.data import DeviceLoader, RandomPadCropFlip, TensorTaskDataset, load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import finetune
    root = str(tmp_path)
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=1, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="mem1")
    dsets = load_task_datasets(ds.get_task_dataset_path("1"), DEV)
    torch.manual_seed(0)
    base = os.path.join(root, "base.pth.tar")
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), base)
    params, epochs = [], []
    for tag in ("padded", "plain"):
        spec = RandomPadCropFlip((32, 32), 0, padding_mode="reflect", p=0.0) if tag == "padded" else None
        per = {s: TensorTaskDataset(dsets[s].x, dsets[s].y, dsets[s].classes, transform=spec) for s in ("train", "val")}
        torch.manual_seed(5)
        epochs.append([(x.clone(), y.clone()) for x, y in DeviceLoader(per["train"], 40, True, DEV)])
        torch.manual_seed(7)
        loaders = {s: DeviceLoader(per[s], 40, True, DEV) for s in per}
        assert (loaders["train"].transform is not None) == (tag == "padded") and tuple(loaders["train"].x.shape[1:]) == (3, 32, 32)
        model, _ = finetune.fine_tune_SGD(loaders, {s: len(per[s]) for s in per}, {s: [per[s].classes] for s in per},
                                          model_path=base, exp_dir=os.path.join(root, tag), num_epochs=1, lr=1e-2, device=DEV,
                                          batch_size=40)
        params.append([p.detach().clone() for p in model.parameters()])
    assert len(epochs[0]) == len(epochs[1]) == 2
    for (xa, ya), (xb, yb) in zip(*epochs):                                         # the plain epoch, bitwise
        assert torch.equal(_bits(xa), _bits(xb)) and torch.equal(ya, yb)
    start = list(torch.load(base, weights_only=False).parameters())
    assert any(not torch.equal(a.cpu(), s) for a, s in zip(params[0], start))        # the epoch did train
    for a, b in zip(*params):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- through the driver
def _friendly_base_model(root):
    """As tests/test_gpu_framework.py: a kaiming classifier init, so that a few epochs move the loss."""
    from clsurvey_amd import models
    torch.manual_seed(0)
    m = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(m, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))


def _common(root, extra):
    return ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "3", "--batch_size", "40", "--saving_freq", "100",
            "--results_root", root, "--synthetic", "2,4,160,40,40,32"] + extra


def _ewc(root, extra):
    from clsurvey_amd.framework import driver
    _friendly_base_model(root)
    driver.main(_common(root, extra) + ["--method_name", "SI", "--runmode", "first_task_basemodel_dump"])
    return driver.main(_common(root, extra) + ["--method_name", "EWC", "--test", "--drop_margin", "0.05"])


def _model_files(root):
    out = {}
    for d, _, files in os.walk(os.path.join(root, "train")):
        for f in files:
            if f == "best_model.pth.tar":
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def _finite(accs):
    return len(accs) > 0 and all(a == a and 0.0 <= a <= 100.0 for a in accs)


VARIANTS = [(["--pad_mode", "reflect"], "reflect", False), (["--u8_frames"], "constant", True)]


def _check_files(root, mode, u8):
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip
    data = os.path.join(root, "data", "synthetic_tiny_imagenet")
    assert sorted(f for f in os.listdir(data) if f.endswith(".pth.tar")) == ["task_1_rndtrans.pth.tar", "task_2_rndtrans.pth.tar"]
    t1 = torch.load(os.path.join(data, "task_1_rndtrans.pth.tar"), weights_only=False)
    t = t1["train"].transform
    assert isinstance(t, RandomPadCropFlip) and (t.size, t.padding, t.padding_mode) == ((32, 32), (4, 4, 4, 4), mode)
    assert t.fill == (128 if u8 else 0.0) and isinstance(t1["train"], ByteTaskDataset) == u8
    assert tuple(t1["train"].x.shape[1:]) == (3, 32, 32) and t1["test"].transform is None and tuple(t1["test"].x.shape[1:]) == (3, 32, 32)


@pytest.mark.parametrize("extra,mode,u8", VARIANTS, ids=["reflect", "u8_frames"])
def test_ewc_through_the_driver_on_padded_tasks(tmp_path, extra, mode, u8):
    """SI dump, LR grid, a Fisher pass over a padded reg_sets loader, evaluation on the static test split."""
    root = str(tmp_path)
    out = _ewc(root, ["--rnd_pad", "4"] + extra)
    _check_files(root, mode, u8)
    res = out["results"]
    assert sorted(res) == [0, 1] and len(res[0]["seq_res"][0]) == 2 and len(res[1]["seq_res"][1]) == 1
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("EWC on padded tasks:", accs)
    assert _finite(accs)
    tdir = os.path.join(out["manager"].parent_exp_dir, "task_2", "TASK_TRAINING")
    assert os.path.exists(os.path.join(tdir, "SUCCESS.FLAG")) and os.path.exists(os.path.join(tdir, "best_model.pth.tar"))
    om = torch.load(os.path.join(tdir, "best_model.pth.tar"), weights_only=False).reg_params
    assert any(float(v["omega"].abs().max()) > 0 for k, v in om.items() if isinstance(v, dict) and "omega" in v)
    assert os.listdir(out["args"].out_path)


@pytest.mark.parametrize("extra,mode,u8", VARIANTS, ids=["reflect", "u8_frames"])
def test_joint_through_the_driver_on_padded_tasks(tmp_path, extra, mode, u8):
    from clsurvey_amd.framework import driver
    root = str(tmp_path)
    _friendly_base_model(root)
    out = driver.main(_common(root, ["--rnd_pad", "4"] + extra) + ["--method_name", "joint", "--test"])
    _check_files(root, mode, u8)
    assert all(os.path.basename(p).endswith("_rndtrans.pth.tar") for p in out["ds_paths"]) and len(out["ds_paths"]) == 2
    accs = out["results"]["joint"]["seq_res"]
    print("joint on padded tasks:", accs)
    assert len(accs) == 2 and _finite(accs)
    assert os.path.exists(out["model_paths"][0]) and os.listdir(out["args"].out_path)


def test_pad_zero_is_a_run_without_the_flag(tmp_path):
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    _ewc(a, ["--rnd_pad", "0"])
    _ewc(b, [])
    fa, fb = _model_files(a), _model_files(b)
    assert len(fa) >= 2 and sorted(fa) == sorted(fb)
    for name in fa:
        assert fa[name] == fb[name], name
    names = sorted(os.listdir(os.path.join(a, "data", "synthetic_tiny_imagenet")))
    assert names == sorted(os.listdir(os.path.join(b, "data", "synthetic_tiny_imagenet"))) and not any("rndtrans" in n for n in names)
