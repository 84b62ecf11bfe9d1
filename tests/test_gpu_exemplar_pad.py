"""Padded replay of stored exemplars on the GPU: clhip_rehearsal_assemble_pad_crop_flip and its byte form against the CPU
restatement of torchvision's pad -> crop -> hflip (tests/pad_crop_ref.py, bitwise: a copy), against the loaders' padded gather
over the same store (bitwise: one device body) and, with all pads 0, against the copying assembly; copy and ring rows, repeated
and unaligned launches, launches without one of the runs, the safety rule; RehearsalNet and GemNet with a RandomPadCropFlip spec
(their draws, a run on padded tasks against the RandomCropFlip run on the host-pre-padded split, a byte store against the fp32
run on the decoded split, the pickle); gem_main.main and the driver with the switch."""
import copy
import functools
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pad_crop_ref as ref  # noqa: E402
from kernel_parity import bitwise_equal  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, RING, ROW0, STORE_ROWS, SRC_ROWS = 3, 2, 4, 8, 5
SRC_IDX = [4, 0]
GATHER = [7, 0, 3, 6, 7, 1, 2, 0, 6, 3, 1, 2, 7, 0, 6, 3, 1, 2]    # E = 18: two sets of corner_rows; none of the ring rows 4, 5
E = len(GATHER)
CASES = ref.cases()
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _channels(geometry):
    """C in {1, 3}: one channel for every third geometry."""
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
def _case(C, Hs, Ws, th, tw, mode, pads, byte=False):
    """Made once per geometry, mode and store kind and never written to (the launches work on device copies).  params: corner_rows
    over the full frame, then over a smaller extent where the mode takes one."""
    gen = torch.Generator().manual_seed(1000 * Hs + 10 * tw + 100 * ref.MODES.index(mode) + int(byte))

    def frames(n):
        if byte:
            return torch.randint(0, 256, (n, C, Hs, Ws), generator=gen, dtype=torch.uint8)
        return torch.randn((n, C, Hs, Ws), generator=gen)
    params = torch.cat([ref.corner_rows(Hs, Ws, th, tw, pads), ref.corner_rows(*_smaller_extent(Hs, Ws, th, tw, mode, pads), th, tw, pads)])
    assert tuple(params.shape) == (E, 5)
    return dict(geo=(C, Hs, Ws, th, tw), mode=mode, pads=tuple(pads), lut=_random_lut(C, gen) if byte else None,
                fill=torch.randn((C,), generator=gen), x=torch.randn((B, C, th, tw), generator=gen),
                y=torch.randint(0, 20, (B,), generator=gen), src=frames(SRC_ROWS), src_idx=torch.tensor(SRC_IDX),
                store=frames(STORE_ROWS), store_y=torch.randint(0, 20, (STORE_ROWS,), generator=gen),
                gather=torch.tensor(GATHER, dtype=torch.int32), params=params.contiguous())


def _launch(c, b=B, ring=RING, e=E, x_mix="new", offset=0, crop=False, lut="own", fill="own"):
    """Runs the entry of case c's store kind on device copies (crop: the unpadded copying assembly, params' first three columns);
    returns the device tensors (store, store_y, x_mix, y_mix, the guard floats in front of x_mix) and the device lut."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = c["geo"]
    byte = c["store"].dtype == torch.uint8
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm = ym = buf = None
    if x_mix is not None:
        buf = torch.full((offset + (b + e) * C * th * tw,), -7.0, device=DEV)
        xm = buf[offset:]
        assert xm.data_ptr() % 16 == 4 * offset
        ym = torch.full((b + e,), 99, dtype=torch.int64, device=DEV)
    table = () if not byte else ((d["lut"] if lut == "own" else lut),)
    params = d["params"][:e].contiguous() if e else None
    rest = (d["x"][:b].contiguous() if x_mix is not None else None, d["y"], b, d["src"], d["src_idx"], d["store"], d["store_y"], ROW0,
            ring, d["gather"][:e] if e else None, params, xm, ym)
    if crop:
        (ops.rehearsal_assemble_crop_flip_u8 if byte else ops.rehearsal_assemble_crop_flip)(c["geo"], *table, *rest)
    else:
        (ops.rehearsal_assemble_pad_crop_flip_u8 if byte else ops.rehearsal_assemble_pad_crop_flip)(
            c["geo"], c["mode"], c["pads"], d["fill"] if fill == "own" else fill, *table, *rest)
    torch.cuda.synchronize()
    return d["store"], d["store_y"], None if xm is None else xm.view(b + e, C, th, tw), ym, None if buf is None else buf[:offset], d.get("lut")


def _decoded(store, lut):
    """CPU fp32 frames a store means."""
    store = store.cpu()
    if store.dtype != torch.uint8:
        return store
    lut = lut.cpu()
    return torch.stack([lut[ch][store[:, ch].long()] for ch in range(store.shape[1])], 1)


def _gathered(c, store, store_y, lut, rows, params):
    """The loaders' padded gather over a one-task table laid over the store: (x [n, C, th, tw], labels [n])."""
    from clsurvey_amd import ops
    table = ops.task_table([store], [store_y], [store.shape[0]], [0], DEV)
    idx, params, fill = rows.to(DEV).long(), params.to(DEV).contiguous(), c["fill"].to(DEV)
    if store.dtype == torch.uint8:
        return ops.gather_tasks_pad_crop_flip_u8(table, c["geo"], c["mode"], c["pads"], fill, lut, idx, params)
    return ops.gather_tasks_pad_crop_flip(table, c["geo"], c["mode"], c["pads"], fill, idx, params)


def _check_copy_and_ring(c, got, b=B, ring=RING):
    """The copy rows, the ring rows and their labels are the inputs bit for bit; the rest of the store is untouched."""
    store, store_y, xm, ym = (None if v is None else v.cpu() for v in got[:4])
    keep = [r for r in range(STORE_ROWS) if not ROW0 <= r < ROW0 + ring]
    assert torch.equal(store[keep].view(-1).view(torch.uint8), c["store"][keep].view(-1).view(torch.uint8))
    assert torch.equal(store_y[keep], c["store_y"][keep])
    want = c["src"][SRC_IDX[:ring]]
    assert torch.equal(store[ROW0:ROW0 + ring].view(-1).view(torch.uint8), want.view(-1).view(torch.uint8))
    assert torch.equal(store_y[ROW0:ROW0 + ring], c["y"][:ring])
    if xm is not None:
        assert bitwise_equal(xm[:b], c["x"][:b]) and torch.equal(ym[:b], c["y"][:b])


# ---------------------------------------------------------------------------------------------- the kernel
def test_the_geometries_still_split_into_the_blocks_they_were_chosen_for():
    from clsurvey_amd import _lib
    rpb = _lib.lib().clhip_crop_rows_per_block
    assert rpb(64) == 64 and -(-70 // rpb(64)) == 2                 # 72 x 72 -> 70 x 64: two chunks of lines, the last one short
    assert rpb(4100) == 1                                           # a line longer than a block's segment
    assert {g[:4] for g in ref.GEOMETRIES} >= {(72, 72, 70, 64), (5, 4200, 2, 4100), (8, 8, 12, 12), (5, 4, 8, 8)}


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("geometry,mode,pads", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_exemplar_rows_are_the_restatement_and_the_gather_bitwise(geometry, mode, pads, byte):
    """Every geometry of the padded gather's tests under every mode it takes; 3 current rows, 2 ring rows, 18 exemplar rows over
    the corner windows of the full frame and of a smaller extent.  The exemplar rows are the CPU restatement of pad -> crop ->
    flip over the (decoded) store and the loaders' gather over the store (one device body); everything else is a copy."""
    Hs, Ws, th, tw = geometry[:4]
    c = _case(_channels(geometry), Hs, Ws, th, tw, mode, pads, byte)
    got = _launch(c)
    _check_copy_and_ring(c, got)
    want = ref.restate(_decoded(got[0], got[5]), c["gather"].long(), c["params"], th, tw, mode, c["fill"].tolist())
    assert got[2].dtype == torch.float32 and bitwise_equal(got[2][B:], want)
    assert torch.equal(got[3][B:].cpu(), c["store_y"][c["gather"].long()])
    gx, gy = _gathered(c, got[0], got[1], got[5], c["gather"], c["params"])
    assert bitwise_equal(got[2][B:], gx) and torch.equal(got[3][B:], gy)
    assert not bool((got[2] == -7.0).any())


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_byte_entry_is_the_fp32_entry_on_the_decoded_store(mode):
    c = _case(3, 20, 20, 16, 16, mode, (4, 4, 4, 4), True)
    got = _launch(c)
    f = dict(c, lut=None, src=_decoded(c["src"], c["lut"]), store=_decoded(c["store"], c["lut"]))
    want = _launch(f)
    assert bitwise_equal(got[2], want[2]) and torch.equal(got[3], want[3]) and torch.equal(got[1], want[1])
    assert bitwise_equal(_decoded(got[0], got[5]), want[0])
    assert torch.equal(got[0][ROW0:ROW0 + RING].cpu(), c["src"][SRC_IDX])             # the stored bytes are the source frames' bytes


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("mode", ref.MODES)
def test_copy_and_ring_rows_are_the_copying_assemblys(mode, byte):
    """Same x, frames, ring and store: the copy rows, the store and every label but the exemplars' windows are those of
    clhip_rehearsal_assemble_crop_flip[_u8] (its windows lie inside the frame)."""
    c = _case(3, 20, 20, 16, 16, mode, (4, 4, 4, 4), byte)
    got = _launch(c)
    inside = dict(c, params=torch.tensor([[k % 5, (3 * k) % 5, k & 1] for k in range(E)], dtype=torch.int32))
    want = _launch(inside, crop=True)
    assert bitwise_equal(got[2][:B], want[2][:B]) and torch.equal(got[3], want[3])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    _check_copy_and_ring(c, got)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("C,Hs,Ws,th,tw", [(3, 20, 20, 16, 16), (1, 13, 11, 8, 7), (3, 72, 72, 70, 64)],
                         ids=["20x20_to_16x16", "13x11_to_8x7", "two_chunks"])
def test_with_all_pads_zero_the_launch_is_the_copying_assembly_bitwise(C, Hs, Ws, th, tw, mode, byte):
    """Pads 0 and full extents: x_mix, the labels and the store are those of clhip_rehearsal_assemble_crop_flip[_u8] for (top,
    left, flip), in every mode.  A -0.0 survives."""
    c = dict(_case(C, Hs, Ws, th, tw, mode, (0, 0, 0, 0), byte))
    c["store"] = c["store"].clone()
    if byte:
        c["store"][7, 0, 0, 0] = 1                                  # byte 1 means -0.0 (_random_lut)
    else:
        c["store"][7, 0, 0, 0] = -0.0
    assert GATHER[0] == 7 and c["params"][0].tolist() == [0, 0, 0, Hs, Ws]
    full = torch.cat([c["params"][:9], c["params"][:9]])            # (the smaller extent's corners are not the crop entry's)
    c["params"] = full.contiguous()
    got = _launch(c)
    want = _launch(dict(c, params=full[:, :3].contiguous()), crop=True)
    assert bitwise_equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool(torch.signbit(got[2][B, 0, 0, 0])) and float(got[2][B, 0, 0, 0]) == 0.0


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("mode", ["constant", "reflect"])
def test_two_launches_are_bitwise_equal_and_an_unaligned_x_mix_takes_the_plain_path(mode, byte):
    """tw % 4 == 0 and x_mix 4 bytes off a 16-byte boundary: no vector stores, the same values, nothing in front of the buffer."""
    c = _case(3, 20, 20, 16, 16, mode, (4, 4, 4, 4), byte)
    a, b2, plain = _launch(c), _launch(c), _launch(c, offset=1)
    for other in (b2, plain):
        assert bitwise_equal(a[2], other[2]) and torch.equal(a[3], other[3]) and torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    assert plain[4].tolist() == [-7.0]
    _check_copy_and_ring(c, plain)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_launches_without_one_of_the_runs(byte):
    c = _case(3, 8, 8, 12, 12, "symmetric", (2, 2, 2, 2), byte)     # the crop is larger than the frame
    full = _launch(c)
    none = _launch(c, e=0)                                          # E == 0: no exemplar blocks
    _check_copy_and_ring(c, none)
    assert none[2].shape[0] == B and torch.equal(none[0], full[0])
    no_fill = _launch(c, e=0, fill=None, lut=None)                  # ... and then neither fill nor table is needed
    assert bitwise_equal(no_fill[2], none[2]) and torch.equal(no_fill[0], none[0])
    no_ring = _launch(c, ring=0)
    _check_copy_and_ring(c, no_ring, ring=0)
    assert torch.equal(no_ring[0].cpu(), c["store"]) and bitwise_equal(no_ring[2], full[2]) and torch.equal(no_ring[3], full[3])
    cc = dict(c, x=c["x"][:0])
    alone = _launch(cc, b=0, ring=0)                                # no current rows
    assert alone[2].shape[0] == E and bitwise_equal(alone[2], full[2][B:]) and torch.equal(alone[3], full[3][B:])


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("geo", [(3, 8, 8, 12, 12), (3, 20, 20, 16, 16)], ids=["crop_larger_than_frame", "20x20_to_16x16"])
def test_the_ring_update_alone_takes_no_x_mix_no_fill_and_no_table(geo, byte):
    """E = 0 and x_mix = NULL: GEM's fill_buffer.  The store rows and labels move, nothing else is touched."""
    c = _case(*geo, "reflect", (2, 2, 2, 2), byte)
    got = _launch(c, e=0, x_mix=None, lut=None, fill=None)
    assert got[2] is None and got[3] is None
    _check_copy_and_ring(c, got)
    assert not torch.equal(got[0].cpu(), c["store"])


BAD_GEO, BAD_PADS = (2, 12, 12, 8, 8), (4, 4, 3, 3)                  # pads (left, top, right, bottom)
BAD = {                                                              # kind -> (mode, what the good row (0, 1, 1, 10, 9) becomes)
    "gather_row": ("constant", None), "gather_row_negative": ("edge", None), "src_idx": ("constant", None),
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
    """One bad row between good ones: its x_mix row keeps the prefill and gets label -1 (src_idx: its store row keeps its frame
    and gets store label -1); every other row is what the launch of the good table gives.  The pads-over-the-limit rows are
    inside every other range: in constant and edge mode the same rows are good."""
    mode, change = BAD[bad]
    ok = copy.deepcopy(_case(*BAD_GEO, mode, BAD_PADS, byte))
    k = 9
    ok["params"][k] = torch.tensor([0, 1, 1, 10, 9], dtype=torch.int32)
    c = copy.deepcopy(ok)
    if bad == "gather_row":
        c["gather"][k] = STORE_ROWS
    elif bad == "gather_row_negative":
        c["gather"][k] = -1
    elif bad == "src_idx":
        c["src_idx"][1] = SRC_ROWS
    else:
        for col, v in change.items():
            c["params"][k, col] = v
    if bad.endswith(("pad_over_h", "pad_over_w")):                  # only the mode's limit makes this row bad
        t, l, _, h, w = c["params"][k].tolist()
        assert 1 <= h <= 12 and 1 <= w <= 12 and -4 <= t <= h + 3 - 8 and -4 <= l <= w + 3 - 8
        plain = _launch(dict(c, mode="edge"))
        assert int(plain[3][B + k]) == int(c["store_y"][c["gather"][k]]) and not bool((plain[2][B + k] == -7.0).any())
    got, want = [v.cpu() for v in _launch(c)[:4]], [v.cpu() for v in _launch(ok)[:4]]
    if bad == "src_idx":
        want[0][ROW0 + 1], want[1][ROW0 + 1] = c["store"][ROW0 + 1], -1
    else:
        want[2][B + k], want[3][B + k] = -7.0, -1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bitwise_equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert not bool((want[2][:B + k] == -7.0).any()) and not bool((want[2][B + k + 1:] == -7.0).any())


def test_argument_errors_come_before_any_launch():
    from clsurvey_amd import _lib, ops
    c = _case(3, 20, 20, 16, 16, "reflect", (4, 4, 4, 4))
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm = torch.full((B + E, 3, 16, 16), -7.0, device=DEV)
    ym = torch.full((B + E,), 99, dtype=torch.int64, device=DEV)
    store0 = d["store"].clone()

    def call(geo=c["geo"], mode="reflect", pads=c["pads"], fill=d["fill"], b=B, row0=ROW0, ring=RING, params=d["params"]):
        ops.rehearsal_assemble_pad_crop_flip(geo, mode, pads, fill, d["x"], d["y"], b, d["src"], d["src_idx"], d["store"], d["store_y"],
                                             row0, ring, d["gather"], params, xm, ym)
    for kw in (dict(row0=-1), dict(row0=STORE_ROWS - RING + 1), dict(b=-1, ring=0), dict(mode=4), dict(mode=-1), dict(pads=(4, -1, 4, 4)),
               dict(pads=(4, 4, 32768, 4))):
        with pytest.raises(_lib.ClhipError, match="CLHIP_EINVAL"):
            call(**kw)
    with pytest.raises(AssertionError, match="fill"):
        call(fill=None)
    with pytest.raises(AssertionError):                             # the crop entry's table has another shape
        call(params=d["params"][:, :3].contiguous())
    with pytest.raises(ValueError):
        call(mode="wrap")
    torch.cuda.synchronize()
    assert bool((xm == -7.0).all()) and bool((ym == 99).all()) and torch.equal(d["store"], store0)


# ---------------------------------------------------------------------------------------------- the wrappers
HW, PAD, NCLS, N_TRAIN, BATCH, N_MEM = 16, 2, 4, 24, 8, 5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL, FILL_BYTES = (0.25, -0.5, 1.0), (128, 3, 250)
CLASSES = [str(k) for k in range(NCLS)]
KINDS = [("partial", False), ("partial", True), ("full", False), ("full", True), ("gem", False)]
KIND_IDS = ["R-PM-fused", "R-PM-segmented", "R-FM-fused", "R-FM-segmented", "GEM"]


def _net():
    """As test_gpu_exemplar_resized._net."""
    from clsurvey_amd.models import VGGSlim
    return VGGSlim(cfg=[8, "M", 16, "M"], num_classes=NCLS, classifier_inputdim=16 * 4 * 4, classifier_dim1=32, classifier_dim2=32,
                   dropout=True, batch_norm=False)


def _padded(mode="constant", fill=FILL, extents=None, p=0.5):
    from clsurvey_amd.data import RandomPadCropFlip
    return RandomPadCropFlip((HW, HW), PAD, fill=fill, padding_mode=mode, p=p, extents=extents)


@functools.lru_cache(maxsize=None)
def _float_tasks(extents=False):
    """Two float tasks of 24 frames 3 x 16 x 16 (CPU) and, with `extents`, a valid extent of its own per frame in [14, 16]."""
    gen = torch.Generator().manual_seed(31 + int(extents))
    out = []
    for _ in range(2):
        y = torch.randint(0, NCLS, (N_TRAIN,), generator=gen)
        x = torch.randn((N_TRAIN, 3, HW, HW), generator=gen) + (y[:, None, None, None] - 1.5) * 0.5
        ext = torch.randint(HW - 2, HW + 1, (N_TRAIN, 2), generator=gen) if extents else None
        out.append((x, y, ext))
    return out


def _padded_dsets(mode, extents=False):
    from clsurvey_amd.data import TensorTaskDataset
    return [TensorTaskDataset(x.to(DEV), y.to(DEV), CLASSES, transform=_padded(mode, extents=ext)) for x, y, ext in _float_tasks(extents)]


def _prepadded_dsets(mode, extents=False):
    """The same tasks with every frame's valid part padded on the host (by indexing: the whole padded image is a window of
    pad_crop_ref) into frames of 20 x 20, top-left anchored, under RandomCropFlip with the padded extents."""
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
    their decoded twins, on the device."""
    from clsurvey_amd.data import ByteTaskDataset
    gen = torch.Generator().manual_seed(21)
    out = []
    for _ in range(2):
        y = torch.randint(0, NCLS, (N_TRAIN,), generator=gen)
        x = (torch.randn((N_TRAIN, 3, HW, HW), generator=gen) * 40 + 128 + (y[:, None, None, None] - 1.5) * 25)
        ext = torch.randint(HW - 2, HW + 1, (N_TRAIN, 2), generator=gen)
        byte = ByteTaskDataset(x.round().clamp(0, 255).to(torch.uint8).to(DEV), y.to(DEV), CLASSES, MEAN, STD,
                               transform=_padded(fill=FILL_BYTES, extents=ext))
        out.append((byte, byte.decoded()))
    return out


def _wrapper(kind, spec, frame_hw, byte=False, segmented=False):
    from clsurvey_amd.methods.gem import GemNet, extend_head
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    torch.manual_seed(5)
    kw = dict(exemplar_transform=spec, frame_shape=(3, frame_hw, frame_hw))
    if byte:
        kw["frame_norm"] = (MEAN, STD)
    if kind == "gem":
        return GemNet(extend_head(_net(), 2 * NCLS), 2 * NCLS, 2, [NCLS] * 2, N_MEM, lr=0.02, memory_strength=0.5, batch_size=BATCH,
                      in_shape=(3, HW, HW), device=DEV, **kw)
    w = RehearsalNet(replace_head(_net(), 2 * NCLS), 2 * NCLS, 2, [NCLS] * 2, N_MEM, 0.02, 1e-4, kind == "full", BATCH + 3,
                     (3, HW, HW), DEV, **kw)
    w.force_segmented = segmented
    return w


def _store(w):
    from clsurvey_amd.methods.gem import GemNet
    if isinstance(w, GemNet):
        return w.memory_x.view((-1,) + w.frame_shape), w.memory_labels.view(-1), w.memory_ext.view(-1, 2)
    return w.store_x, w.store_y, w.store_ext


def _step(w, loader, x, t, y):
    from clsurvey_amd.methods.exemplar import batch_source
    from clsurvey_amd.methods.gem import GemNet
    src = batch_source(loader)
    return w.observe(x, t, y, source=src) if isinstance(w, GemNet) else w.observe_FT(x, t, y, source=src)


def _run(w, dsets, steps=3):
    """Two tasks, `steps` steps each, from a fixed RNG state.  Returns per step (loss, hits, parameters, gather rows, draws)."""
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.gem import GemNet
    torch.manual_seed(9)
    random.seed(9)
    trace = []
    for t, dset in enumerate(dsets):
        if not isinstance(w, GemNet):
            w.init_setup(lr=0.02, weight_decay=1e-4, n_append=3 if t else 0, chunk_size=2)
        loader = DeviceLoader(dset, BATCH, True, DEV)
        for k, (x, y) in enumerate(loader):
            if k == steps:
                break
            out = _step(w, loader, x, t, y)
            hits = out[1].clone() if torch.is_tensor(out[1]) else out[1]
            trace.append((out[0].clone(), hits, [p.detach().clone() for p in w.parameters()], copy.copy(w.__dict__.get("last_gather")),
                          w.__dict__.get("last_exemplar_params")))
    torch.cuda.synchronize()
    return trace


def _same_traces(ta, tb, draws=None):
    """draws(da, db): what two steps' exemplar draws must satisfy (default: equal)."""
    assert len(ta) == len(tb) == 6
    for (la, ha, pa, ga, da), (lb, hb, pb, gb, db) in zip(ta, tb):
        assert bitwise_equal(la.reshape(1), lb.reshape(1)) and bool(torch.isfinite(la).all())
        if torch.is_tensor(ha):
            assert torch.equal(ha, hb)
        for p, q in zip(pa, pb):
            assert bitwise_equal(p, q)
        assert ga == gb and (da is None) == (db is None)
        if da is not None:
            assert torch.equal(da, db) if draws is None else draws(da, db)
    assert any(not torch.equal(p, q) for p, q in zip(ta[0][2], ta[-1][2]))          # the steps did train


def _planned_step(w, dset, seed=13):
    """One step at task 1 with the plan's seeds recorded.  Returns (x, y, seeds)."""
    from clsurvey_amd.data import DeviceLoader
    seen, orig = [], w.plan

    def plan(t, seeds=None):
        out = orig(t, seeds)
        seen[:] = list(seeds)
        return out
    w.plan = plan
    torch.manual_seed(seed)
    random.seed(seed)
    loader = DeviceLoader(dset, BATCH, True, DEV)
    x, y = next(iter(loader))
    _step(w, loader, x, 1, y)
    del w.plan
    return x, y, seen


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_a_rehearsal_step_replays_the_draws_of_its_seed(byte):
    """After RehearsalNet.observe_FT: last_exemplar_params is draw_pad_crop_flip over store_ext[last_gather] from the seed the plan
    handed out, and x_mix[B:N] is the CPU restatement of pad -> crop -> flip over the (decoded) store rows for those draws."""
    from clsurvey_amd.data import draw_pad_crop_flip, norm_lut
    tasks = [d[0 if byte else 1] for d in _byte_tasks()]
    spec = _padded(fill=FILL_BYTES if byte else tasks[0].transform.fill)
    w = _wrapper("partial", spec, HW, byte=byte)
    _run(w, tasks[:1], steps=3)
    w.init_setup(lr=0.02, weight_decay=1e-4, n_append=3, chunk_size=2)
    x, y, seeds = _planned_step(w, tasks[1])
    rows, params = w.last_gather, w.last_exemplar_params
    assert len(rows) == 3 and all(0 <= r < N_MEM for r in rows) and tuple(params.shape) == (3, 5) and params.dtype == torch.int32
    ext = w.store_ext[torch.tensor(rows)]
    assert int(ext.min()) >= HW - 2 and int(ext.max()) <= HW and torch.equal(params[:, 3:].long(), ext)
    want = draw_pad_crop_flip(3, _padded(extents=ext), (HW, HW), torch.Generator().manual_seed(seeds[-1]))
    assert torch.equal(params, want)
    lut = norm_lut(*w.frame_norm) if byte else None
    fill = [float(lut[c, v]) for c, v in enumerate(FILL_BYTES)] if byte else list(spec.fill)
    assert w.fill.tolist() == torch.tensor(fill, dtype=torch.float32).tolist()
    want_x = ref.restate(_decoded(w.store_x, lut), torch.tensor(rows), params, HW, HW, "constant", fill)
    assert bitwise_equal(w.x_mix[BATCH:BATCH + 3], want_x) and torch.equal(w.y_mix[BATCH:BATCH + 3].cpu(), w.store_y.cpu()[rows])
    assert bitwise_equal(w.x_mix[:BATCH], x) and torch.equal(w.y_mix[:BATCH], y)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("mode", ["constant", "symmetric"])
def test_gems_memory_pass_replays_the_draws_of_its_seed(mode, byte):
    """GemNet's memory loader carries the spec (the byte store's with its byte fill) and the memory's extents; the batch it serves
    is the CPU restatement over memory[0] for draw_pad_crop_flip from the loader's base seed."""
    from clsurvey_amd.data import ByteTaskDataset, RandomPadCropFlip, draw_pad_crop_flip, norm_lut
    tasks = [d[0 if byte else 1] for d in _byte_tasks()]
    fill = FILL_BYTES if byte else tasks[0].transform.fill
    tasks = [copy.copy(d) for d in tasks]
    for d in tasks:
        d.transform = _padded(mode, fill, d.transform.extents, p=0.25)
    w = _wrapper("gem", _padded(mode, fill, p=0.25), HW, byte=byte)
    _run(w, tasks, steps=1)
    torch.manual_seed(17)
    loader = w._memory_loader(0)
    t = loader.transform
    assert isinstance(t, RandomPadCropFlip) and (t.size, t.padding, t.fill, t.padding_mode, t.p) == ((HW, HW), (PAD,) * 4, fill, mode, 0.25)
    assert torch.equal(t.extents, w.memory_ext[0]) and int(t.extents.min()) < HW
    assert isinstance(loader.dataset, ByteTaskDataset) == byte and loader._padded
    x, y = next(iter(loader))
    order = loader.last_idx_host
    assert sorted(order.tolist()) == list(range(N_MEM))
    params = draw_pad_crop_flip(N_MEM, t, (HW, HW), torch.Generator().manual_seed(loader.base_seed), order=order)
    lut = norm_lut(*w.frame_norm) if byte else None
    fill_f = [float(lut[c, v]) for c, v in enumerate(FILL_BYTES)] if byte else list(fill)
    want = ref.restate(_decoded(w.memory_x[0], lut), order, params, HW, HW, mode, fill_f)
    assert bitwise_equal(x, want) and torch.equal(y.cpu(), w.memory_labels[0].cpu()[order])


@pytest.mark.parametrize("extents", [False, True], ids=["full_frames", "own_extents"])
@pytest.mark.parametrize("mode", ["constant", "reflect"])
@pytest.mark.parametrize("kind,segmented", KINDS, ids=KIND_IDS)
def test_a_run_on_padded_tasks_is_the_crop_run_on_the_host_prepadded_split(kind, segmented, mode, extents):
    """draw_pad_crop_flip's i is draw_crop_flip's top on the padded extent, so the loaders' and the exemplars' draws line up:
    losses, hits and parameters of every step are bitwise those of the frame-mode RandomCropFlip run on frames padded on the
    host, and the store holds the unpadded frames of the same samples."""
    a = _wrapper(kind, _padded(mode), HW, segmented=segmented)
    ta = _run(a, _padded_dsets(mode, extents))
    from clsurvey_amd.data import RandomCropFlip
    b = _wrapper(kind, RandomCropFlip((HW, HW), 0.5), HW + 2 * PAD, segmented=segmented)
    tb = _run(b, _prepadded_dsets(mode, extents))
    assert type(a.exemplar_transform).__name__ == "RandomPadCropFlip" and type(b.exemplar_transform).__name__ == "RandomCropFlip"

    def draws(da, db):
        return da.shape[1] == 5 and db.shape[1] == 3 and torch.equal(da[:, :2] + PAD, db[:, :2]) and torch.equal(da[:, 2], db[:, 2])
    _same_traces(ta, tb, draws)
    (ax, ay, aext), (bx, by, bext) = _store(a), _store(b)
    assert torch.equal(ay, by) and torch.equal(aext + 2 * PAD, bext) and (int(aext.min()) < HW) == extents
    for n in range(ax.shape[0]):                                    # the valid parts are the same pixels
        h, w = aext[n].tolist()
        assert bitwise_equal(ax[n, :, :h, :w], bx[n, :, PAD:PAD + h, PAD:PAD + w])
    if kind != "gem":
        assert a.last_path == b.last_path == ("segmented" if segmented else "fused")
        assert int(a.last_exemplar_params[:, :2].min()) >= -PAD
        assert bitwise_equal(a.x_mix[:BATCH + 3], b.x_mix[:BATCH + 3]) and torch.equal(a.y_mix[:BATCH + 3], b.y_mix[:BATCH + 3])


@pytest.mark.parametrize("kind", ["partial", "gem"])
def test_a_byte_store_run_is_the_fp32_run_on_the_decoded_split(kind):
    from clsurvey_amd.data import norm_lut
    tasks = _byte_tasks()
    a = _wrapper(kind, _padded(fill=FILL_BYTES), HW, byte=True)
    ta = _run(a, [byte for byte, _ in tasks])
    b = _wrapper(kind, _padded(fill=tasks[0][1].transform.fill), HW)
    tb = _run(b, [dec for _, dec in tasks])
    assert a.frame_norm is not None and b.frame_norm is None and a.store_dtype == torch.uint8
    assert bitwise_equal(a.fill, b.fill) and a.exemplar_transform.fill == FILL_BYTES
    _same_traces(ta, tb)
    (bx, by, bext), (fx, fy, fext) = _store(a), _store(b)
    assert bx.dtype == torch.uint8 and int(bx.max()) > 0 and bitwise_equal(_decoded(bx, norm_lut(*a.frame_norm)), fx)
    assert torch.equal(by, fy) and torch.equal(bext, fext) and int(bext.min()) < HW
    if kind != "gem":
        assert tuple(a.last_exemplar_params.shape) == (3, 5)
        assert bitwise_equal(a.x_mix[:BATCH + 3], b.x_mix[:BATCH + 3]) and torch.equal(a.y_mix[:BATCH + 3], b.y_mix[:BATCH + 3])


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("kind", ["partial", "gem"])
def test_pickle_round_trip_gives_the_same_next_step(kind, byte):
    from clsurvey_amd.data import DeviceLoader, RandomPadCropFlip
    tasks = [d[0 if byte else 1] for d in _byte_tasks()]
    fill = FILL_BYTES if byte else tasks[0].transform.fill
    w = _wrapper(kind, _padded(fill=fill), HW, byte=byte)
    _run(w, tasks, steps=2)
    buf = io.BytesIO()
    torch.save(w, buf)
    buf.seek(0)
    w2 = torch.load(buf, weights_only=False)
    t = w2.exemplar_transform
    assert isinstance(t, RandomPadCropFlip) and t.extents is None and w2.params_width == 5
    assert (t.size, t.padding, t.fill, t.padding_mode, t.p) == ((HW, HW), (PAD,) * 4, fill, "constant", 0.5)
    assert w2.fill is not w.fill and w2.fill.is_cuda and bitwise_equal(w2.fill, w.fill)          # rebuilt by _bind, not pickled
    for u, v in zip(_store(w2), _store(w)):
        assert u.dtype == v.dtype and torch.equal(u, v)
    res = []
    for v in (w, w2):
        if kind == "gem":
            v.init_setup(lr=0.02, weight_decay=0.0, memory_strength=0.5)
        else:
            v.init_setup(lr=0.02, weight_decay=1e-4, n_append=3, chunk_size=2)      # what main() does after torch.load
        torch.manual_seed(13)
        random.seed(13)
        loader = DeviceLoader(tasks[1], BATCH, True, DEV)
        x, y = next(iter(loader))
        out = _step(v, loader, x, 1, y)
        res.append((out[0].clone(), [p.detach().clone() for p in v.parameters()], v.__dict__.get("last_exemplar_params")))
    assert bitwise_equal(res[0][0].reshape(1), res[1][0].reshape(1))
    for p, q in zip(res[0][1], res[1][1]):
        assert bitwise_equal(p, q)
    if kind != "gem":
        assert torch.equal(res[0][2], res[1][2]) and tuple(res[0][2].shape) == (3, 5)


def test_gems_fill_buffer_takes_a_crop_larger_than_the_frame():
    """Frames of 12 x 12 under RandomCrop(16, padding=2): the ring-only launch copies the frames, a memory pass serves 16 x 16."""
    from clsurvey_amd.data import DeviceLoader, RandomPadCropFlip, TensorTaskDataset
    from clsurvey_amd.methods.exemplar import batch_source
    from clsurvey_amd.methods.gem import GemNet, extend_head
    gen = torch.Generator().manual_seed(3)
    spec = RandomPadCropFlip((HW, HW), PAD, padding_mode="edge")
    x, y = torch.randn((N_TRAIN, 3, HW - 4, HW - 4), generator=gen), torch.randint(0, NCLS, (N_TRAIN,), generator=gen)
    dset = TensorTaskDataset(x.to(DEV), y.to(DEV), CLASSES, transform=spec)
    torch.manual_seed(5)
    w = GemNet(extend_head(_net(), 2 * NCLS), 2 * NCLS, 2, [NCLS] * 2, N_MEM, lr=0.02, memory_strength=0.5, batch_size=BATCH,
               in_shape=(3, HW, HW), device=DEV, exemplar_transform=spec, frame_shape=(3, HW - 4, HW - 4))
    loader = DeviceLoader(dset, BATCH, True, DEV)
    xb, yb = next(iter(loader))
    w.init_new_task(0)
    assert w.fill_buffer(0, xb, yb, batch_source(loader)) is True
    idx = loader.last_idx_host[:N_MEM]
    assert bitwise_equal(w.memory_x[0], x[idx]) and torch.equal(w.memory_labels[0].cpu(), y[idx])
    mx, my = next(iter(w._memory_loader(0)))
    assert tuple(mx.shape) == (N_MEM, 3, HW, HW) and bool(torch.isfinite(mx).all())


# ---------------------------------------------------------------------------------------------- gem_main.main
def _seeds(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _dicts(root, byte, mode="reflect"):
    """The padded files of two synthetic tasks (frames 3 x 32 x 32, pad 2), loaded to the device."""
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="pd", u8_frames=byte, rnd_pad=2, pad_mode=mode)
    return [load_task_datasets(ds.get_task_dataset_path(str(t), rnd_transform=True), DEV) for t in (1, 2)]


def _base_model(path):
    from clsurvey_amd import models
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), path)
    return path


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_rehearsal_partial_mem_entry_builds_then_loads_with_the_switch(tmp_path, byte):
    from clsurvey_amd.data import RandomPadCropFlip
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dicts = _dicts(root, byte)
    assert all(isinstance(d["train"].transform, RandomPadCropFlip) for d in dicts)
    prev = _base_model(os.path.join(root, "prev.pth.tar"))
    common = dict(n_outputs=8, method="baseline_rehearsal_partial_mem", n_memories=6, n_tasks=2, postprocess=False, n_epochs=1,
                  batch_size=16, lr=1e-2, exemplar_padded=True, **({"exemplar_dtype": "uint8"} if byte else {}))
    dt = torch.uint8 if byte else torch.float32
    first = dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0], is_scratch_model=True,
                 save_path=os.path.join(root, "t1"))
    with pytest.raises(NotImplementedError, match="padded replay is not built"):
        gem_main.main({k: v for k, v in first.items() if k != "exemplar_padded"}, [4, 4], device=DEV)
    _seeds(11)
    m1, acc1 = gem_main.main(first, [4, 4], device=DEV)
    assert isinstance(m1.exemplar_transform, RandomPadCropFlip) and m1.exemplar_transform.padding_mode == "reflect"
    assert m1.store_x.dtype == dt and tuple(m1.store_x.shape) == (12, 3, 32, 32) and m1.filled == [6, 0] and 0.0 <= acc1 <= 1.0
    assert float(m1.store_x[:6].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and float(m1.store_x[6:].float().abs().sum()) == 0
    saved = os.path.join(root, "t1", "best_model.pth.tar")
    m2, acc2 = gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=saved, dataset_path=dicts[1],
                                  is_scratch_model=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert isinstance(m2.exemplar_transform, RandomPadCropFlip) and m2.store_x.dtype == dt
    assert m2.filled == [6, 6] and m2.last_path == "fused" and len(m2.last_gather) > 0 and 0.0 <= acc2 <= 1.0
    assert tuple(m2.last_exemplar_params.shape) == (len(m2.last_gather), 5)
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_gem_entry_builds_then_loads_with_the_switch(tmp_path, byte):
    from clsurvey_amd.data import RandomPadCropFlip
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dicts = _dicts(root, byte, mode="constant")
    prev = _base_model(os.path.join(root, "SI", "prev.pth.tar"))
    common = dict(n_outputs=8, method="gem", n_memories=6, n_tasks=2, n_epochs=1, batch_size=16, lr=1e-2, memory_strength=0.5,
                  exemplar_padded=True, **({"exemplar_dtype": "uint8"} if byte else {}))
    dt = torch.uint8 if byte else torch.float32
    _seeds(12)
    wrapped = os.path.join(root, "t1", "best_model.pth.tar")
    gem_main.main(dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0], is_scratch_model=True,
                       postprocess=True, save_path=wrapped), [4, 4], device=DEV)
    w = torch.load(wrapped, weights_only=False)
    assert isinstance(w.exemplar_transform, RandomPadCropFlip) and (w.frame_norm is not None) == byte
    assert w.exemplar_transform.fill == (128 if byte else 0.0)
    assert w.memory_x.dtype == dt and tuple(w.memory_x.shape) == (2, 6, 3, 32, 32)
    assert float(w.memory_x[0].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and float(w.memory_x[1].float().abs().sum()) == 0
    m2, acc2 = gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=wrapped, dataset_path=dicts[1],
                                  is_scratch_model=False, postprocess=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert m2.memory_x.dtype == dt and m2.observed_tasks == [0, 1] and 0.0 <= acc2 <= 1.0
    assert float(m2.memory_x[1].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and torch.equal(m2.memory_x[0], w.memory_x[0])
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())


# ---------------------------------------------------------------------------------------------- through the driver
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_rehearsal_partial_mem_through_the_driver_on_padded_tasks(tmp_path, byte):
    from clsurvey_amd import models
    from clsurvey_amd.data import RandomPadCropFlip
    from clsurvey_amd.framework import driver
    root = str(tmp_path)
    torch.manual_seed(0)
    m = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(m, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))
    argv = ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "2", "--batch_size", "40", "--saving_freq", "100",
            "--results_root", root, "--synthetic", "2,4,160,40,40,32", "--rnd_pad", "2", "--pad_mode", "reflect", "--padded_exemplars",
            "--method_name", "finetuning_rehearsal_partial_mem", "--test", "--mem_per_task", "24"]
    if byte:
        argv += ["--u8_frames", "--u8_exemplars"]
    out = driver.main(argv)
    res = out["results"]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("R-PM on padded tasks:", accs)
    assert sorted(res) == [0, 1] and len(accs) > 0 and all(a == a and 0.0 <= a <= 100.0 for a in accs)
    for k, path in enumerate(out["model_paths"], start=1):
        w = torch.load(path, weights_only=False)
        assert isinstance(w.exemplar_transform, RandomPadCropFlip) and w.exemplar_transform.size == (32, 32)
        assert w.exemplar_transform.padding == (2, 2, 2, 2) and w.exemplar_transform.padding_mode == "reflect"
        assert w.store_x.dtype == (torch.uint8 if byte else torch.float32) and tuple(w.store_x.shape) == (48, 3, 32, 32)
        assert w.filled[:k] == [24] * k and (w.frame_norm is not None) == byte
        assert float(w.store_x[:24 * k].float().abs().sum(dim=(1, 2, 3)).min()) > 0
