"""iCaRL on padded RandomCrop tasks, on the GPU.  clhip_icarl_assemble_pad_crop_flip and its byte form against the CPU
restatement of torchvision's pad -> crop -> hflip (tests/pad_crop_ref.py) and against the loaders' padded gather over the same
store (one device body), the target run over more than one block, the byte entry against the fp32 entry on the decoded store,
zero pads against clhip_icarl_assemble_crop_flip, launches without one of the runs, unaligned and repeated launches, the safety
rule and the argument errors; IcarlNet with a RandomPadCropFlip spec against the crop-frame wrapper on the host-pre-padded split,
against a restatement of its own draws, a byte store against the fp32 run on the decoded split, the pickle; icarl_main.main with
exemplar_pad_frames and ICARL through the driver with --icarl_padded.  Nothing here computes: every comparison is bitwise."""
import copy
import functools
import io
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pad_crop_ref as ref  # noqa: E402
from kernel_parity import bitwise_equal  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, STORE_ROWS = 3, 8                                               # (the store tensors carry one spare row behind store_rows)
GATHER = [7, 0, 3, 6, 7, 1, 2, 0, 6, 3, 1, 2, 7, 0, 6, 3, 1, 2]    # E = 18: two sets of corner_rows; store row 7 three times
E = len(GATHER)
GUARD = 4                                                          # guard floats before and after an output (keeps 16-byte alignment)
SENTINEL = -7.0
CASES = ref.cases()
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
EINVAL = -1


def _channels(geometry):
    """C in {1, 3}: one channel for every third geometry (test_gpu_exemplar_pad._channels)."""
    return 1 if ref.GEOMETRIES.index(geometry) % 3 == 1 else 3


def _random_lut(C, gen):
    """fp32 [C][256] of random values with +0.0, -0.0 and a denormal among them."""
    lut = torch.randn((C, 256), generator=gen)
    lut[:, 0], lut[:, 1] = 0.0, -0.0
    lut[:, 2] = torch.tensor([1], dtype=torch.int32).view(torch.float32)
    return lut


def _smaller_extent(Hs, Ws, th, tw, mode, pads):
    """An extent below the frame's that the mode and the crop still take, else the frame's own."""
    pl, pt, pr, pb = pads
    h, w = max(Hs - 1, 1), max(Ws - 2, 1)
    lim_h, lim_w = ref.pad_limit(mode, h), ref.pad_limit(mode, w)
    ok = h + pt + pb >= th and w + pl + pr >= tw and (lim_h is None or (max(pt, pb) <= lim_h and max(pl, pr) <= lim_w))
    return (h, w) if ok else (Hs, Ws)


@functools.lru_cache(maxsize=None)
def _case(C, Hs, Ws, th, tw, mode, pads, byte=False, n_out=12):
    """Made once per geometry, mode, store kind and target width and never written to (the launches work on device copies).
    params: corner_rows over the full frame, then over a smaller extent where the mode takes one.  A byte case's fill is what its
    fill bytes mean: lut[c, fill byte of c]."""
    gen = torch.Generator().manual_seed(1000 * Hs + 10 * tw + 100 * ref.MODES.index(mode) + int(byte) + 7 * n_out)
    params = torch.cat([ref.corner_rows(Hs, Ws, th, tw, pads), ref.corner_rows(*_smaller_extent(Hs, Ws, th, tw, mode, pads), th, tw, pads)])
    assert tuple(params.shape) == (E, 5)
    if byte:
        store = torch.randint(0, 256, (STORE_ROWS + 1, C, Hs, Ws), generator=gen, dtype=torch.uint8)
        lut = _random_lut(C, gen)
        fill_bytes = torch.randint(0, 256, (C,), generator=gen)
        fill = lut[torch.arange(C), fill_bytes].clone()
    else:
        store, lut = torch.randn((STORE_ROWS + 1, C, Hs, Ws), generator=gen), None
        fill = torch.randn((C,), generator=gen)
    return dict(geo=(C, Hs, Ws, th, tw), mode=mode, pads=tuple(pads), n_out=n_out, lut=lut, fill=fill, store=store,
                x=torch.randn((B, C, th, tw), generator=gen), y=torch.randint(1, 20, (B,), generator=gen),
                store_t=torch.randn((STORE_ROWS + 1, n_out), generator=gen),
                gather=torch.tensor(GATHER, dtype=torch.int32), params=params.contiguous())


def _decoded(store, lut):
    """CPU fp32 frames a store means (indexing, no arithmetic)."""
    store = store.cpu()
    if store.dtype != torch.uint8:
        return store
    lut = lut.cpu()
    return torch.stack([lut[ch][store[:, ch].long()] for ch in range(store.shape[1])], 1)


def _guarded(n, offset=0):
    """A device buffer of n floats with GUARD floats (and `offset` more in front) around it, all SENTINEL; (whole, view)."""
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + n]
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def _launch(c, b=B, e=E, off_x=0, off_t=0, null_x=False, crop=False, lut="own", fill="own"):
    """Runs the entry of case c's store kind on device copies (crop: clhip_icarl_assemble_crop_flip[_u8] with the params' first
    three columns).  Returns CPU (x_mix [b + e, C, th, tw], y_mix, t_mix [b + e, n_out]) after checking that the guard floats
    around x_mix and t_mix are untouched."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = c["geo"]
    byte = c["store"].dtype == torch.uint8
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    row = C * th * tw
    xbuf, xm = _guarded((b + e) * row, off_x)
    tbuf, tm = _guarded((b + e) * c["n_out"], off_t)
    ym = torch.full((b + e,), 99, dtype=torch.int64, device=DEV)
    table = () if not byte else ((d["lut"] if lut == "own" else lut),)
    rest = (None if null_x else d["x"][:b].contiguous(), None if null_x else d["y"], b, d["store"][:STORE_ROWS],
            d["gather"][:e] if e else None, d["params"][:e].contiguous() if e else None, d["store_t"], xm, ym,
            tm.view(b + e, c["n_out"]))
    if crop:
        (ops.icarl_assemble_crop_flip_u8 if byte else ops.icarl_assemble_crop_flip)(c["geo"], *table, *rest)
    else:
        (ops.icarl_assemble_pad_crop_flip_u8 if byte else ops.icarl_assemble_pad_crop_flip)(
            c["geo"], c["mode"], c["pads"], d["fill"] if fill == "own" else fill, *table, *rest)
    torch.cuda.synchronize()
    for buf, n, off in ((xbuf, (b + e) * row, off_x), (tbuf, (b + e) * c["n_out"], off_t)):
        host = buf.cpu()
        assert bool((host[:GUARD + off] == SENTINEL).all()) and bool((host[GUARD + off + n:] == SENTINEL).all())
    return xm.cpu().view(b + e, C, th, tw), ym.cpu(), tm.cpu().view(b + e, c["n_out"])


def _expect(c, b=B, e=E):
    """(x_mix, y_mix, t_mix) of a launch over case c: the copy rows, the CPU restatement of pad -> crop -> flip over the decoded
    store, zeros for the exemplar labels, the stored target rows behind b rows of prefill."""
    C, Hs, Ws, th, tw = c["geo"]
    rows = c["gather"][:e].long()
    if e == 0:
        ex = torch.zeros((0, C, th, tw))
    else:
        ex = ref.restate(_decoded(c["store"], c["lut"]), rows, c["params"][:e], th, tw, c["mode"], c["fill"].tolist())
    return (torch.cat([c["x"][:b], ex]), torch.cat([c["y"][:b], torch.zeros(e, dtype=torch.int64)]),
            torch.cat([torch.full((b, c["n_out"]), SENTINEL), c["store_t"].index_select(0, rows)]))


def _gathered(c, rows, params):
    """The loaders' padded gather over a one-task table laid over the store: crops [n, C, th, tw] (CPU)."""
    from clsurvey_amd import ops
    store = c["store"].to(DEV)
    table = ops.task_table([store], [torch.zeros(store.shape[0], dtype=torch.int64, device=DEV)], [store.shape[0]], [0], DEV)
    idx, params, fill = rows.to(DEV).long(), params.to(DEV).contiguous(), c["fill"].to(DEV)
    if c["lut"] is not None:
        return ops.gather_tasks_pad_crop_flip_u8(table, c["geo"], c["mode"], c["pads"], fill, c["lut"].to(DEV), idx, params)[0].cpu()
    return ops.gather_tasks_pad_crop_flip(table, c["geo"], c["mode"], c["pads"], fill, idx, params)[0].cpu()


def _same(got, want):
    """Tuples of CPU tensors, equal in shape, type and every byte."""
    return all(g.shape == w.shape and g.dtype == w.dtype and
               torch.equal(g.contiguous().view(-1).view(torch.uint8), w.contiguous().view(-1).view(torch.uint8)) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("geometry,mode,pads", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_exemplar_rows_are_the_restatement_and_the_gather_bitwise(geometry, mode, pads, byte):
    """Every geometry of the padded gather's tests under every mode it takes; 3 current rows, 18 exemplar rows over the corner
    windows of the full frame and of a smaller extent, store row 7 three times.  x_mix[B:] is the CPU restatement over the
    (decoded) store and the loaders' gather over the store; labels 0; t_mix[B + e] = store_t[gather[e]]; the copy rows are the
    inputs; the guard floats stay (checked in _launch)."""
    Hs, Ws, th, tw = geometry[:4]
    c = _case(_channels(geometry), Hs, Ws, th, tw, mode, pads, byte)
    got = _launch(c)
    assert _same(got, _expect(c))
    assert bitwise_equal(got[0][B:], _gathered(c, c["gather"], c["params"]))
    assert got[1][B:].tolist() == [0] * E and torch.equal(got[1][:B], c["y"]) and bitwise_equal(got[0][:B], c["x"])
    assert bitwise_equal(got[2][B:], c["store_t"][c["gather"].long()])
    assert bitwise_equal(got[2][B], got[2][B + 4]) and GATHER[0] == GATHER[4]          # one target row, twice
    assert not bool((got[0] == SENTINEL).any())


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("n_out", [460, 118, 12, 5], ids=["vec_two_blocks", "scalar_two_blocks", "vec", "scalar"])
def test_the_target_run_over_two_blocks_and_small_rows(n_out, byte):
    """A target block moves 1024 accesses: 9 rows of 460 floats are 9 x 115 float4 > 1024, 9 rows of 118 floats 1062 scalar
    accesses > 1024; 12 and 5 floats stay inside one block."""
    c = _case(3, 20, 20, 16, 16, "reflect", (4, 4, 4, 4), byte, n_out)
    assert 9 * (n_out // 4 if n_out % 4 == 0 else n_out) > 1024 or n_out < 100
    got = _launch(c, e=9)
    assert _same(got, _expect(c, e=9))
    assert bitwise_equal(got[2][B:], c["store_t"][c["gather"][:9].long()])


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_byte_entry_is_the_fp32_entry_on_the_decoded_store(mode):
    c = _case(3, 20, 20, 16, 16, mode, (4, 4, 4, 4), True)
    f = dict(c, lut=None, store=_decoded(c["store"], c["lut"]))     # (c's fill is lut[c, fill byte] already)
    assert _same(_launch(c), _launch(f))


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("C,Hs,Ws,th,tw", [(3, 20, 20, 16, 16), (1, 13, 11, 8, 7), (3, 72, 72, 70, 64)],
                         ids=["20x20_to_16x16", "13x11_to_8x7", "two_chunks"])
def test_with_all_pads_zero_the_launch_is_the_crop_assembly_bitwise(C, Hs, Ws, th, tw, mode, byte):
    """Pads 0 and full extents: x_mix, the labels and t_mix are those of clhip_icarl_assemble_crop_flip[_u8] for (top, left,
    flip), in every mode."""
    c = dict(_case(C, Hs, Ws, th, tw, mode, (0, 0, 0, 0), byte))
    full = torch.cat([c["params"][:9], c["params"][:9]])            # (the smaller extent's corners are not the crop entry's)
    assert full[:, 3:].tolist() == [[Hs, Ws]] * E
    c["params"] = full.contiguous()
    assert _same(_launch(c), _launch(dict(c, params=full[:, :3].contiguous()), crop=True))


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_launches_without_one_of_the_runs(byte):
    """B = 0 with x = labels = NULL (the class-mean view's form); E = 0 is a plain copy and needs neither fill nor table."""
    c = _case(3, 8, 8, 12, 12, "symmetric", (2, 2, 2, 2), byte)     # the crop is larger than the frame
    full = _launch(c)
    assert _same(full, _expect(c))
    alone = _launch(c, b=0, null_x=True)
    assert _same(alone, _expect(c, b=0)) and _same(alone, tuple(v[B:] for v in full))
    assert _same(_launch(c, b=0), _expect(c, b=0))
    none = _launch(c, e=0)
    assert _same(none, _expect(c, e=0)) and none[0].shape[0] == B
    assert _same(_launch(c, e=0, fill=None, lut=None), none)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_two_launches_are_bitwise_equal_and_unaligned_outputs_take_the_plain_paths(mode, byte):
    """tw % 4 == 0 and n_outputs % 4 == 0, but x_mix / t_mix 4 bytes off a 16-byte boundary: no 16-byte accesses, the same
    values, the floats around them untouched."""
    c = _case(3, 20, 20, 16, 16, mode, (4, 4, 4, 4), byte)
    want = _expect(c)
    a = _launch(c)
    assert _same(a, want) and _same(_launch(c), a)
    assert _same(_launch(c, off_x=1), want) and _same(_launch(c, off_t=1), want) and _same(_launch(c, off_x=1, off_t=1), want)


BAD_GEO, BAD_PADS = (2, 12, 12, 8, 8), (4, 4, 3, 3)                  # pads (left, top, right, bottom)
BAD = {                                                              # kind -> (mode, what the good row (0, 1, 1, 10, 9) becomes)
    "gather_row": ("constant", None), "gather_row_negative": ("edge", None),
    "flip": ("constant", {2: 2}), "flip_negative": ("edge", {2: -1}),
    "h_zero": ("constant", {3: 0}), "h_past_the_frame": ("edge", {3: 13}), "h_int_max": ("constant", {3: I32_MAX}),
    "w_zero": ("edge", {4: 0}), "w_past_the_frame": ("constant", {4: 13}), "w_negative": ("edge", {4: -5}),
    "top_below": ("constant", {0: -5}), "top_above": ("edge", {0: 10 + 3 - 8 + 1}), "top_int_min": ("reflect", {0: I32_MIN}),
    "top_int_max": ("symmetric", {0: I32_MAX}),
    "left_below": ("edge", {1: -5}), "left_above": ("constant", {1: 9 + 3 - 8 + 1}), "left_int_min": ("symmetric", {1: I32_MIN}),
    "left_int_max": ("reflect", {1: I32_MAX}),
    "reflect_pad_over_h": ("reflect", {0: -3, 3: 4}), "reflect_pad_over_w": ("reflect", {1: -3, 4: 4}),
    "symmetric_pad_over_h": ("symmetric", {0: -3, 3: 3}), "symmetric_pad_over_w": ("symmetric", {1: -3, 4: 3}),
}


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_rows_copy_nothing_and_get_label_minus_one(bad, byte):
    """One bad row between good ones: its x_mix row AND its t_mix row keep the sentinel and it gets label -1; every other row is
    the restatement of the good table.  The pads-over-the-limit rows are inside every other range: in edge mode the same rows
    are good.  Target rows of 12 floats (16-byte accesses) and of 5 (scalar).  (The store tensors carry a spare row and every
    buffer is allocated at full size: a kernel without the rule would read inside this test's allocations and fail by value.)"""
    mode, change = BAD[bad]
    k = 9
    for n_out in (12, 5):
        ok = copy.deepcopy(_case(*BAD_GEO, mode, BAD_PADS, byte, n_out))
        ok["params"][k] = torch.tensor([0, 1, 1, 10, 9], dtype=torch.int32)
        c = copy.deepcopy(ok)
        if bad == "gather_row":
            c["gather"][k] = STORE_ROWS
        elif bad == "gather_row_negative":
            c["gather"][k] = -1
        else:
            for col, v in change.items():
                c["params"][k, col] = v
        if bad.endswith(("pad_over_h", "pad_over_w")) and n_out == 12:      # only the mode's limit makes this row bad
            t, l, _, h, w = c["params"][k].tolist()
            assert 1 <= h <= 12 and 1 <= w <= 12 and -4 <= t <= h + 3 - 8 and -4 <= l <= w + 3 - 8
            plain = _launch(dict(c, mode="edge"))
            assert int(plain[1][B + k]) == 0 and not bool((plain[0][B + k] == SENTINEL).any())
        want = [v.clone() for v in _expect(ok)]
        want[0][B + k], want[1][B + k], want[2][B + k] = SENTINEL, -1, SENTINEL
        assert _same(_launch(c), want)
        assert not bool((want[0][:B + k] == SENTINEL).any()) and not bool((want[0][B + k + 1:] == SENTINEL).any())


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_argument_errors_come_before_any_launch(byte):
    """Each refused call returns CLHIP_EINVAL and leaves x_mix, y_mix and t_mix as they were."""
    from clsurvey_amd import _lib
    from clsurvey_amd.ops import _stream
    c = _case(3, 20, 20, 16, 16, "reflect", (4, 4, 4, 4), byte)
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm = torch.full((B + E, 3, 16, 16), SENTINEL, device=DEV)
    ym = torch.full((B + E,), 99, dtype=torch.int64, device=DEV)
    tm = torch.full((B + E, 12), SENTINEL, device=DEV)
    f = getattr(_lib.lib(), "clhip_icarl_assemble_pad_crop_flip" + ("_u8" if byte else ""))
    PAD_MAX, PAD_MAX_EXTENT = 32767, 1 << 30

    def call(geo=c["geo"], mode=2, pads=c["pads"], fill=d["fill"].data_ptr(), lut="own", b=B, e=E, store_t=d["store_t"].data_ptr()):
        table = ((d["lut"].data_ptr() if lut == "own" else lut),) if byte else ()
        return f(d["x"].data_ptr(), d["y"].data_ptr(), b, *geo, mode, *pads, fill, *table, d["store"].data_ptr(), STORE_ROWS,
                 d["gather"].data_ptr(), d["params"].data_ptr(), e, store_t, 12, xm.data_ptr(), ym.data_ptr(), tm.data_ptr(), _stream())
    refused = [dict(mode=4), dict(mode=-1), dict(pads=(4, -1, 4, 4)), dict(pads=(4, 4, PAD_MAX + 1, 4)),
               dict(geo=(3, PAD_MAX_EXTENT + 1, 20, 16, 16)), dict(geo=(3, 20, PAD_MAX_EXTENT + 1, 16, 16)), dict(fill=None),
               dict(store_t=None), dict(b=65535 - E + 1)]
    if byte:
        refused.append(dict(lut=None))
    for kw in refused:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((xm == SENTINEL).all()) and bool((ym == 99).all()) and bool((tm == SENTINEL).all())
    assert call() == 0                                               # ... and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert _same((xm.cpu(), ym.cpu(), tm.cpu()[B:]), tuple(v if i < 2 else v[B:] for i, v in enumerate(_expect(c))))


# ---------------------------------------------------------------------------------------------- the wrapper
HW, PAD, NCLS, N_TRAIN, BATCH, N_MEM, N_APPEND, HERD_BATCH, EVAL_BATCH = 16, 4, 4, 24, 8, 8, 3, 5, 3
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL, FILL_BYTES = (0.25, -0.5, 1.0), (128, 3, 250)
CLASSES = [str(k) for k in range(NCLS)]


def _net():
    """As test_gpu_icarl_augment._net."""
    from clsurvey_amd.models import VGGSlim
    return VGGSlim(cfg=[8, "M", 16, "M"], num_classes=NCLS, classifier_inputdim=16 * 4 * 4, classifier_dim1=32, classifier_dim2=32,
                   dropout=True, batch_norm=False)


def _padded(mode="constant", fill=FILL, extents=None, p=0.5):
    from clsurvey_amd.data import RandomPadCropFlip
    return RandomPadCropFlip((HW, HW), PAD, fill=fill, padding_mode=mode, p=p, extents=extents)


@functools.lru_cache(maxsize=None)
def _float_tasks(extents=False):
    """Two float tasks of 24 frames 3 x 16 x 16 (CPU), 6 images per class, and, with `extents`, a valid extent of its own per
    frame in [14, 16]."""
    gen = torch.Generator().manual_seed(41 + int(extents))
    out = []
    for _ in range(2):
        y = torch.arange(N_TRAIN)[torch.randperm(N_TRAIN, generator=gen)] % NCLS
        x = torch.randn((N_TRAIN, 3, HW, HW), generator=gen) + (y[:, None, None, None] - 1.5) * 0.5
        ext = torch.randint(HW - 2, HW + 1, (N_TRAIN, 2), generator=gen) if extents else None
        out.append((x, y, ext))
    return out


def _padded_dsets(mode, extents=False):
    from clsurvey_amd.data import TensorTaskDataset
    return [TensorTaskDataset(x.to(DEV), y.to(DEV), CLASSES, transform=_padded(mode, extents=ext)) for x, y, ext in _float_tasks(extents)]


def _prepadded_dsets(mode, extents=False):
    """The same tasks with every frame's valid part padded on the host (by indexing: the whole padded image is a window of
    pad_crop_ref) into frames of 24 x 24, top-left anchored, under RandomCropFlip with the padded extents."""
    from clsurvey_amd.data import RandomCropFlip, TensorTaskDataset
    out = []
    for x, y, ext in _float_tasks(extents):
        xp = torch.zeros((N_TRAIN, 3, HW + 2 * PAD, HW + 2 * PAD))
        for n in range(N_TRAIN):
            h, w = (HW, HW) if ext is None else ext[n].tolist()
            xp[n, :, :h + 2 * PAD, :w + 2 * PAD] = ref.window(x[n], -PAD, -PAD, 0, h, w, h + 2 * PAD, w + 2 * PAD, mode, FILL)
        spec = RandomCropFlip((HW, HW), 0.5, extents=None if ext is None else ext + 2 * PAD)
        out.append(TensorTaskDataset(xp.to(DEV), y.to(DEV), CLASSES, transform=spec))
    return out


@functools.lru_cache(maxsize=None)
def _byte_tasks():
    """Two byte tasks under the constant padded spec with a byte fill per channel, each frame with an extent of its own, and
    their decoded twins, on the device: [(byte split, decoded split)]."""
    from clsurvey_amd.data import ByteTaskDataset
    gen = torch.Generator().manual_seed(23)
    out = []
    for _ in range(2):
        y = torch.arange(N_TRAIN)[torch.randperm(N_TRAIN, generator=gen)] % NCLS
        x = (torch.randn((N_TRAIN, 3, HW, HW), generator=gen) * 40 + 128 + (y[:, None, None, None] - 1.5) * 25)
        ext = torch.randint(HW - 2, HW + 1, (N_TRAIN, 2), generator=gen)
        byte = ByteTaskDataset(x.round().clamp(0, 255).to(torch.uint8).to(DEV), y.to(DEV), CLASSES, MEAN, STD,
                               transform=_padded(fill=FILL_BYTES, extents=ext))
        out.append((byte, byte.decoded()))
    return out


def _wrapper(spec, frame_hw, segmented=False, byte=False):
    from clsurvey_amd.methods.icarl import IcarlNet
    torch.manual_seed(5)
    kw = dict(exemplar_transform=spec, frame_shape=(3, frame_hw, frame_hw))
    if byte:
        kw["frame_norm"] = (MEAN, STD)
    w = IcarlNet(_net(), 2 * NCLS, 2, [NCLS] * 2, N_MEM, lr=0.02, weight_decay=1e-4, memory_strength=1.0, batch_size=BATCH + N_APPEND,
                 in_shape=(3, HW, HW), device=DEV, **kw)
    w.force_segmented = segmented
    return w


def _seed(v):
    torch.manual_seed(v)
    random.seed(v)
    np.random.seed(v)


def _setup(w, t):
    w.init_setup(lr=0.02, weight_decay=1e-4, memory_strength=1.0, n_append=N_APPEND if t else 0, chunk_size=BATCH, total_batch_size=2)


def _herd_args(dset):
    return types.SimpleNamespace(task_imgfolders={"train": dset}, batch_size=HERD_BATCH)


def _run(w, dsets, steps=3, after_step=None, after_herding=None):
    """Two tasks from a fixed RNG state: `steps` observe steps each, then manage_memory.  Returns per step (loss, parameters,
    gather rows, draws) and per task (ranking, herding draws)."""
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.exemplar import batch_source
    _seed(9)
    trace, herds = [], []
    for t, dset in enumerate(dsets):
        _setup(w, t)
        loader = DeviceLoader(dset, BATCH, True, DEV)
        for k, (x, y) in enumerate(loader):
            if k == steps:
                break
            before = (torch.get_rng_state(), np.random.get_state(), random.getstate())
            out = w.observe(x, t, y, source=batch_source(loader))
            trace.append((out[0].clone(), [p.detach().clone() for p in w.parameters()], list(w.last_gather), w.last_exemplar_params))
            if after_step is not None:
                after_step(w, t, x, y, before)
        w.manage_memory(t, _herd_args(dset))
        herds.append((w.last_ranking[0].cpu().tolist(), w.last_herd_params))
        if after_herding is not None:
            after_herding(w, t, dset)
    torch.cuda.synchronize()
    return trace, herds


@functools.lru_cache(maxsize=None)
def _probe():
    return torch.randn((7, 3, HW, HW), generator=torch.Generator().manual_seed(77)).to(DEV)


def _codes(w):
    args = types.SimpleNamespace(batch_size=EVAL_BATCH)
    return torch.stack([w(_probe(), t, args=args).cpu() for t in range(2)])


def _same_traces(ta, tb, draws=None):
    """draws(da, db): what two steps' exemplar draws must satisfy (default: equal)."""
    assert len(ta) == len(tb) == 6
    for (la, pa, ga, da), (lb, pb, gb, db) in zip(ta, tb):
        assert bitwise_equal(la.reshape(1), lb.reshape(1)) and bool(torch.isfinite(la).all())
        for p, q in zip(pa, pb):
            assert bitwise_equal(p, q)
        assert ga == gb
        assert torch.equal(da, db) if draws is None else draws(da, db)
    assert len(ta[-1][2]) == N_APPEND and len(ta[0][2]) == 0
    assert any(not torch.equal(p, q) for p, q in zip(ta[0][1], ta[-1][1]))          # the steps did train


@pytest.mark.parametrize("segmented", [False, True], ids=["fused", "segmented"])
@pytest.mark.parametrize("extents", [False, True], ids=["full_frames", "own_extents"])
@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_a_run_on_padded_tasks_is_the_crop_frame_run_on_the_host_prepadded_split(mode, extents, segmented):
    """draw_pad_crop_flip's corner + pad is draw_crop_flip's corner on the padded extent from the same seed, so the loaders', the
    herding view's, the replays' and the class-mean view's draws line up: losses and parameters of every step, the rankings,
    store_t, the class means and the NME codes are bitwise those of the frame-mode RandomCropFlip wrapper on frames padded on the
    host, and the store holds the unpadded frames of the same samples."""
    from clsurvey_amd.data import RandomCropFlip
    a = _wrapper(_padded(mode), HW, segmented)
    ta, ha = _run(a, _padded_dsets(mode, extents))
    b = _wrapper(RandomCropFlip((HW, HW), 0.5), HW + 2 * PAD, segmented)
    tb, hb = _run(b, _prepadded_dsets(mode, extents))
    assert type(a.exemplar_transform).__name__ == "RandomPadCropFlip" and type(b.exemplar_transform).__name__ == "RandomCropFlip"
    assert a.last_path == b.last_path == ("segmented" if segmented else "fused")

    def draws(da, db):
        return (tuple(da.shape) == (db.shape[0], 5) and db.shape[1] == 3 and torch.equal(da[:, :2] + PAD, db[:, :2]) and
                torch.equal(da[:, 2], db[:, 2]) and (da.shape[0] == 0 or int(da[:, :2].min()) >= -PAD))
    _same_traces(ta, tb, draws)
    for (ra, pa), (rb, pb) in zip(ha, hb):
        assert ra == rb and len(ra) >= NCLS and tuple(pa.shape) == (N_TRAIN, 5) and tuple(pb.shape) == (N_TRAIN, 3)
        assert draws(pa, pb)
    assert -PAD <= int(ha[0][1][:, :2].min()) < 0                   # some herding window does reach into the padding
    assert a.last_gather == b.last_gather and a.class_len == b.class_len == [2] * 8
    assert bitwise_equal(a.store_t, b.store_t) and float(a.store_t.abs().sum()) > 0
    assert bitwise_equal(a.x_mix[:BATCH + N_APPEND], b.x_mix[:BATCH + N_APPEND])
    for t in range(2):
        assert bitwise_equal(a.class_means(t, EVAL_BATCH), b.class_means(t, EVAL_BATCH))
    ca, cb = _codes(a), _codes(b)
    assert torch.equal(ca, cb) and float(ca.sum()) == 2 * 7
    assert tuple(a.store_x.shape) == (2 * N_MEM, 3, HW, HW) and tuple(b.store_x.shape) == (2 * N_MEM, 3, HW + 2 * PAD, HW + 2 * PAD)
    assert torch.equal(a.store_ext + 2 * PAD, b.store_ext) and (int(a.store_ext.min()) < HW) == extents
    ax, bx = a.store_x.cpu(), b.store_x.cpu()
    for n in a.stored_rows():                                       # the valid parts are the same pixels
        h, w = a.store_ext[n].tolist()
        assert bitwise_equal(ax[n, :, :h, :w], bx[n, :, PAD:PAD + h, PAD:PAD + w]) and float(ax[n].abs().sum()) > 0


@pytest.mark.parametrize("mode", ["constant", "symmetric"])
def test_herding_and_replay_follow_their_own_draws(mode):
    """After manage_memory: last_herd_params is draw_pad_crop_flip over the split's extents from view_seed_of(view_seed, t,
    VIEW_HERD).  After every observe: last_exemplar_params is the draw over store_ext[last_gather] from the plan's last seed,
    x_mix[B:N) is the CPU restatement over the store for those draws, t_mix[B:N) is store_t[last_gather], and the global
    generators stand where the crop-mode step's host draws (plan) leave them."""
    from clsurvey_amd.data import draw_pad_crop_flip
    from clsurvey_amd.methods.icarl import VIEW_HERD, view_seed_of
    dsets = _padded_dsets(mode, True)
    w = _wrapper(_padded(mode), HW)
    assert tuple(w.store_x.shape) == (2 * N_MEM, 3, HW, HW) and w.params_width == 5
    assert w.fill.tolist() == torch.tensor(FILL, dtype=torch.float32).tolist()
    seeds_seen, orig, seen = [], w.plan, []

    def plan(t, seeds=None):
        out = orig(t, seeds)
        if seeds is not None:
            seeds_seen[:] = list(seeds)
        return out
    w.plan = plan

    def after_step(w, t, x, y, before):
        n, Ex = x.shape[0], len(w.last_gather)
        assert Ex == (N_APPEND if t else 0) and tuple(w.last_exemplar_params.shape) == (Ex, 5)
        assert bitwise_equal(w.x_mix[:n], x) and torch.equal(w.y_mix[:n], y)
        after = (torch.get_rng_state(), np.random.get_state(), random.getstate())
        torch.set_rng_state(before[0])
        np.random.set_state(before[1])
        random.setstate(before[2])
        orig(t)                                                    # the host draws of a crop-mode step
        assert torch.equal(torch.get_rng_state(), after[0]) and random.getstate() == after[2]
        assert np.array_equal(np.random.get_state()[1], after[1][1]) and np.random.get_state()[2] == after[1][2]
        if Ex:
            ext = w.store_ext[torch.tensor(w.last_gather)]
            want = draw_pad_crop_flip(Ex, _padded(mode, extents=ext), (HW, HW), torch.Generator().manual_seed(seeds_seen[-1]))
            assert torch.equal(w.last_exemplar_params, want) and torch.equal(want[:, 3:].long(), ext)
            want_x = ref.restate(w.store_x.cpu(), torch.tensor(w.last_gather), want, HW, HW, mode, list(FILL))
            assert bitwise_equal(w.x_mix[n:n + Ex], want_x) and int(w.y_mix[n:n + Ex].abs().sum()) == 0
            assert bitwise_equal(w.t_mix[n:n + Ex], w.store_t[torch.tensor(w.last_gather, device=DEV)])
            seen.append(want)

    def after_herding(w, t, dset):
        ext = dset.transform.extents
        want = draw_pad_crop_flip(N_TRAIN, _padded(mode, extents=ext), (HW, HW),
                                  torch.Generator().manual_seed(view_seed_of(w.view_seed, t, VIEW_HERD)))
        assert torch.equal(w.last_herd_params, want) and torch.equal(want, w.view_params(t, VIEW_HERD, ext))
        assert int(want[:, :2].min()) < 0 and int(want[:, :2].min()) >= -PAD

    trace, _ = _run(w, dsets, after_step=after_step, after_herding=after_herding)
    assert len(seen) == 3 and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert all(bool(torch.isfinite(s[0]).all()) for s in trace) and w.last_path == "fused"
    codes = _codes(w)
    w._means = {}
    assert torch.equal(codes, _codes(w)) and float(codes.sum()) == 2 * 7                    # an evaluation is reproducible


def test_a_byte_store_run_is_the_fp32_run_on_the_decoded_split():
    from clsurvey_amd.data import norm_lut
    tasks = _byte_tasks()
    a = _wrapper(_padded(fill=FILL_BYTES), HW, byte=True)
    ta, ha = _run(a, [byte for byte, _ in tasks])
    b = _wrapper(_padded(fill=tasks[0][1].transform.fill), HW)
    tb, hb = _run(b, [dec for _, dec in tasks])
    assert a.frame_norm is not None and b.frame_norm is None and a.store_dtype == torch.uint8 and a.store_x.dtype == torch.uint8
    assert bitwise_equal(a.fill, b.fill) and a.exemplar_transform.fill == FILL_BYTES
    _same_traces(ta, tb)
    for (ra, pa), (rb, pb) in zip(ha, hb):
        assert ra == rb and torch.equal(pa, pb)
    assert bitwise_equal(_decoded(a.store_x, norm_lut(*a.frame_norm)), b.store_x) and int(a.store_x.max()) > 0
    assert torch.equal(a.store_ext, b.store_ext) and int(a.store_ext.min()) < HW and bitwise_equal(a.store_t, b.store_t)
    assert tuple(a.last_exemplar_params.shape) == (N_APPEND, 5)
    assert bitwise_equal(a.x_mix[:BATCH + N_APPEND], b.x_mix[:BATCH + N_APPEND])
    assert torch.equal(_codes(a), _codes(b))


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_pickle_round_trip_gives_the_same_next_step_and_codes(byte):
    from clsurvey_amd.data import DeviceLoader, RandomPadCropFlip
    from clsurvey_amd.methods.exemplar import batch_source
    tasks = [d[0 if byte else 1] for d in _byte_tasks()]
    fill = FILL_BYTES if byte else tasks[0].transform.fill
    w = _wrapper(_padded(fill=fill), HW, byte=byte)
    _run(w, tasks[:1], steps=1)                                     # (saved after task 1)
    w.view_seed = 3
    state = w.__getstate__()
    n = sum(w.class_len)
    assert state["_rows_x"].dtype == w.store_dtype and tuple(state["_rows_x"].shape) == (n, 3, HW, HW) and n == 16
    assert tuple(state["_rows_ext"].shape) == (n, 2) and int(state["_rows_ext"].min()) < HW
    assert not {"store_x", "store_t", "store_ext", "last_gather", "last_exemplar_params", "last_herd_params", "lut", "fill"} & set(state)
    buf = io.BytesIO()
    torch.save(w, buf)
    buf.seek(0)
    w2 = torch.load(buf, weights_only=False)
    t = w2.exemplar_transform
    assert isinstance(t, RandomPadCropFlip) and t.extents is None and w2.params_width == 5 and w2.view_seed == 3
    assert (t.size, t.padding, t.fill, t.padding_mode, t.p) == ((HW, HW), (PAD,) * 4, fill, "constant", 0.5)
    assert w2.fill is not w.fill and w2.fill.is_cuda and bitwise_equal(w2.fill, w.fill)          # rebuilt by _bind, not pickled
    assert (w2.frame_norm is not None) == byte and w2.last_gather is None
    assert torch.equal(w2.store_x, w.store_x) and torch.equal(w2.store_t, w.store_t) and torch.equal(w2.store_ext, w.store_ext)
    codes = [_codes(v) for v in (w, w2)]
    assert torch.equal(codes[0], codes[1])
    res = []
    for v in (w, w2):
        _setup(v, 1)                                               # what main() does after torch.load
        _seed(15)
        loader = DeviceLoader(tasks[1], BATCH, True, DEV)
        x, y = next(iter(loader))
        loss, hits, _ = v.observe(x, 1, y, batch_source(loader))
        Ex = len(v.last_gather)
        res.append((loss.clone(), hits.clone(), v.x_mix[:BATCH + Ex].clone(), v.last_exemplar_params,
                    [p.detach().clone() for p in v.parameters()]))
    assert bitwise_equal(res[0][0].reshape(1), res[1][0].reshape(1)) and torch.equal(res[0][1], res[1][1])
    assert bitwise_equal(res[0][2], res[1][2])
    assert torch.equal(res[0][3], res[1][3]) and tuple(res[0][3].shape) == (N_APPEND, 5)
    for p, q in zip(res[0][4], res[1][4]):
        assert bitwise_equal(p, q)


# ---------------------------------------------------------------------------------------------- icarl_main.main
def _dicts(root, byte, mode="reflect"):
    """The padded files of two synthetic tasks (frames 3 x 32 x 32, pad 4), loaded to the device."""
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="pd", u8_frames=byte, rnd_pad=PAD, pad_mode=mode)
    return [load_task_datasets(ds.get_task_dataset_path(str(t), rnd_transform=True), DEV) for t in (1, 2)]


def _base_model(path):
    from clsurvey_amd import models
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), path)
    return path


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_icarl_entry_builds_then_loads_with_the_switch(tmp_path, byte):
    """Task 1 is the postprocess alone (wrap and herd), task 2 loads the saved wrapper and trains; without the switch the split
    is refused as before, and a loaded crop-frame wrapper is refused with it."""
    from clsurvey_amd import models
    from clsurvey_amd.data import RandomCropFlip, RandomPadCropFlip
    from clsurvey_amd.methods import icarl_main
    from clsurvey_amd.methods.icarl import IcarlNet
    root = str(tmp_path)
    dicts = _dicts(root, byte)
    assert all(isinstance(d["train"].transform, RandomPadCropFlip) for d in dicts)
    prev = _base_model(os.path.join(root, "SI", "prev.pth.tar"))
    common = dict(n_outputs=8, method="icarl", n_memories=8, n_tasks=2, n_epochs=1, batch_size=16, lr=1e-2, memory_strength=1.0,
                  exemplar_pad_frames=True, **({"exemplar_dtype": "uint8"} if byte else {}))
    dt = torch.uint8 if byte else torch.float32
    wrapped = os.path.join(root, "t1", "best_model.pth.tar")
    first = dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0], is_scratch_model=True,
                 postprocess=True, save_path=wrapped)
    with pytest.raises(NotImplementedError, match="padded replay is not built"):
        icarl_main.main({k: v for k, v in first.items() if k != "exemplar_pad_frames"}, [4, 4], device=DEV)
    _seed(12)
    assert icarl_main.main(first, [4, 4], device=DEV) == (None, None)
    w = torch.load(wrapped, weights_only=False)
    assert isinstance(w.exemplar_transform, RandomPadCropFlip) and w.exemplar_transform.padding_mode == "reflect"
    assert w.exemplar_transform.padding == (PAD,) * 4 and (w.frame_norm is not None) == byte
    assert w.store_x.dtype == dt and tuple(w.store_x.shape) == (16, 3, 32, 32) and w.class_len == [4] * 4
    assert float(w.store_x[:16].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and w.last_herd_params is None
    m2, acc2 = icarl_main.main(dict(common, task_name="2", task_count=2, prev_model_path=wrapped, dataset_path=dicts[1],
                                    is_scratch_model=False, postprocess=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert isinstance(m2.exemplar_transform, RandomPadCropFlip) and m2.store_x.dtype == dt and m2.observed_tasks == [0, 1]
    assert len(m2.last_gather) > 0 and tuple(m2.last_exemplar_params.shape) == (len(m2.last_gather), 5) and 0.0 <= acc2 <= 1.0
    assert int(m2.last_exemplar_params[:, :2].min()) >= -PAD and m2.last_path == "fused"
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())
    # a wrapper built in crop-frame mode is not a padded one
    torch.manual_seed(1)
    kw = dict(frame_norm=(dicts[0]["train"].mean, dicts[0]["train"].std)) if byte else {}
    other = IcarlNet(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), 8, 2, [4, 4], 8, lr=1e-2, batch_size=16,
                     in_shape=(3, 32, 32), device=DEV, exemplar_transform=RandomCropFlip((32, 32), 0.5), frame_shape=(3, 36, 36), **kw)
    crop_path = os.path.join(root, "crop", "best_model.pth.tar")
    os.makedirs(os.path.dirname(crop_path))
    torch.save(other, crop_path)
    with pytest.raises(ValueError, match="the loaded wrapper replays"):
        icarl_main.main(dict(common, task_name="2", task_count=2, prev_model_path=crop_path, dataset_path=dicts[1],
                             is_scratch_model=False, postprocess=False, save_path=os.path.join(root, "t3")), [4, 4], device=DEV)


# ---------------------------------------------------------------------------------------------- through the driver
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_icarl_through_the_driver_on_padded_tasks(tmp_path, byte):
    """An SI first-task dump, then two tasks of ICARL --test on a padded synthetic sequence (sized as
    test_icarl_through_the_driver_on_augmented_tasks): the run reaches the end, the accuracies are finite, the saved wrappers
    hold the unpadded frames."""
    from clsurvey_amd import models
    from clsurvey_amd.data import RandomPadCropFlip
    from clsurvey_amd.framework import driver
    from clsurvey_amd.methods import method as M
    root = str(tmp_path)
    torch.manual_seed(0)
    m = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(m, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))
    flags = ["--rnd_pad", str(PAD), "--pad_mode", "reflect", "--icarl_padded"] + (["--u8_frames", "--u8_exemplars"] if byte else [])
    common = ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "3", "--batch_size", "40", "--saving_freq", "100",
              "--results_root", root, "--synthetic", "2,4,160,40,40,32"] + flags
    icarl = M.parse("ICARL")
    icarl.static_hyperparams = {"mem_per_task": 16}
    driver.main(common + ["--method_name", "SI", "--runmode", "first_task_basemodel_dump"])
    out = driver.main(common + ["--method_name", "ICARL", "--test"], method=icarl)
    res = out["results"]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("iCaRL on padded tasks:", {i: res[i]["seq_res"][i] for i in res})
    assert sorted(res) == [0, 1] and len(accs) > 0 and all(np.isfinite(a) and 0.0 <= a <= 100.0 for a in accs)
    dt = torch.uint8 if byte else torch.float32
    assert len(out["model_paths"]) == 2
    for k, path in enumerate(out["model_paths"], start=1):
        w = torch.load(path, weights_only=False)
        count = 32 // (4 * k)
        t = w.exemplar_transform
        assert isinstance(t, RandomPadCropFlip) and t.size == (32, 32) and t.padding == (PAD,) * 4 and t.padding_mode == "reflect"
        assert w.frame_shape == (3, 32, 32) and w.in_shape == (3, 32, 32) and (w.frame_norm is not None) == byte
        assert w.store_dtype == dt and w.store_x.dtype == dt and tuple(w.store_x.shape) == (32, 3, 32, 32)
        assert w.exemplar_count == count and w.class_len == [count] * (4 * k) and w.observed_tasks == list(range(k))
        assert w.store_ext.tolist() == [[32, 32]] * 32
        assert float(w.store_x[:4 * k * count].float().abs().sum(dim=(1, 2, 3)).min()) > 0
