"""Resized replay of stored exemplars on the GPU: clhip_rehearsal_assemble_resized_crop_flip and its byte form against the
loaders' resizing gather over the same store (bitwise: both run one device body), identity windows against the copying assembly
(bitwise), the fp64 restatement of the filter with ATen's own fp32 error as the yardstick, the safety rule and the argument
errors; RehearsalNet and GemNet with a RandomResizedCropFlip spec (their draws, a spec without freedom against the crop run, a
byte store against the fp32 run on the decoded split, the pickle); gem_main.main and the driver with the switch."""
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
import resized_crop_ref as ref  # noqa: E402
from kernel_parity import bitwise_equal  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 4.0          # the rule of test_gpu_resized_crop.py: the kernel's error may be this many times ATen's fp32 CPU error
B, RING, ROW0, STORE_ROWS, SRC_ROWS = 5, 3, 4, 12, 9
SRC_IDX = [7, 0, 3]
GATHER = [9, 0, 3, 11, 9, 1, 8, 2, 7, 10, 0, 11, 3]               # E = 13; none of the ring rows 4 .. 6
E = len(GATHER)
GEOMETRIES = [(1, 5, 7, 8, 8), (3, 40, 33, 8, 8), (2, 9, 9, 4, 12), (3, 64, 64, 56, 56), (2, 64, 64, 8, 8), (3, 12, 10, 5, 7)]
IDS = ["%dx%dx%d_to_%dx%d" % g for g in GEOMETRIES]


def _hand_made(Hs, Ws):
    """The windows of test_gpu_resized_crop.py: 1 x 1 in two corners, the whole frame under both flips, one on each border."""
    h, w = max(1, (2 * Hs) // 3), max(1, (2 * Ws) // 3)
    return [[0, 0, 1, 1, 0], [Hs - 1, Ws - 1, 1, 1, 1], [0, 0, Hs, Ws, 0], [0, 0, Hs, Ws, 1],
            [0, (Ws - w) // 2, h, w, 1], [Hs - h, (Ws - w) // 2, h, w, 0], [(Hs - h) // 2, 0, h, w, 1], [(Hs - h) // 2, Ws - w, h, w, 0]]


def _random_lut(C, gen):
    """fp32 [C][256] of random values with +0.0, -0.0 and a denormal among them."""
    lut = torch.randn((C, 256), generator=gen)
    lut[:, 0], lut[:, 1] = 0.0, -0.0
    lut[:, 2] = torch.tensor([1], dtype=torch.int32).view(torch.float32)
    return lut


@functools.lru_cache(maxsize=None)
def _case(C, Hs, Ws, th, tw, byte=False):
    """Made once per geometry and store kind and never written to (the launches work on device copies)."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    gen = torch.Generator().manual_seed(1000 * Hs + 10 * tw + int(byte))
    if Hs > 8 * th or Ws > 8 * tw:      # a frame the spec's draws refuse (a window could pass CLHIP_RESIZE_MAX_RATIO): windows that do not
        hand = torch.tensor([[k % (Hs - 8 * th + 1), k % (Ws - 8 * tw + 1), 1 + (3 * k) % (8 * th), 1 + (5 * k) % (8 * tw), k & 1]
                             for k in range(E)], dtype=torch.int32)
        drawn = hand[:0]
    else:
        hand = torch.tensor(_hand_made(Hs, Ws), dtype=torch.int32)
        drawn = draw_resized_crop_flip(E - len(hand), RandomResizedCropFlip((th, tw)), (Hs, Ws), gen)

    def frames(n):
        if byte:
            return torch.randint(0, 256, (n, C, Hs, Ws), generator=gen, dtype=torch.uint8)
        return torch.randn((n, C, Hs, Ws), generator=gen)
    return dict(geo=(C, Hs, Ws, th, tw), lut=_random_lut(C, gen) if byte else None,
                x=torch.randn((B, C, th, tw), generator=gen), y=torch.randint(0, 20, (B,), generator=gen),
                src=frames(SRC_ROWS), src_idx=torch.tensor(SRC_IDX), store=frames(STORE_ROWS),
                store_y=torch.randint(0, 20, (STORE_ROWS,), generator=gen),
                gather=torch.tensor(GATHER, dtype=torch.int32), params=torch.cat([hand, drawn]).contiguous())


def _entry(c, crop=False):
    from clsurvey_amd import ops
    byte = c["store"].dtype == torch.uint8
    if crop:
        return ops.rehearsal_assemble_crop_flip_u8 if byte else ops.rehearsal_assemble_crop_flip
    return ops.rehearsal_assemble_resized_crop_flip_u8 if byte else ops.rehearsal_assemble_resized_crop_flip


def _launch(c, b=B, ring=RING, e=E, x_mix="new", offset=0, crop=False, lut="own"):
    """Runs the entry of case c's store kind on device copies; returns the device tensors (store, store_y, x_mix, y_mix, the
    guard floats in front of x_mix) and the device lut."""
    C, Hs, Ws, th, tw = c["geo"]
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm = ym = buf = None
    if x_mix is not None:
        buf = torch.full((offset + (b + e) * C * th * tw,), -7.0, device=DEV)
        xm = buf[offset:]
        assert xm.data_ptr() % 16 == 4 * offset
        ym = torch.full((b + e,), 99, dtype=torch.int64, device=DEV)
    table = () if c["lut"] is None else ((d["lut"] if lut == "own" else lut),)
    _entry(c, crop)(c["geo"], *table, d["x"][:b].contiguous() if x_mix is not None else None, d["y"], b, d["src"], d["src_idx"],
                    d["store"], d["store_y"], ROW0, ring, d["gather"][:e] if e else None, d["params"][:e] if e else None, xm, ym)
    torch.cuda.synchronize()
    return d["store"], d["store_y"], None if xm is None else xm.view(b + e, C, th, tw), ym, None if buf is None else buf[:offset], d.get("lut")


def _gathered(c, store, store_y, lut, rows, params):
    """The loaders' resizing gather over a one-task table laid over the store: (x [n, C, th, tw], labels [n])."""
    from clsurvey_amd import ops
    table = ops.task_table([store], [store_y], [store.shape[0]], [0], DEV)
    idx, params = rows.to(DEV).long(), params.to(DEV).contiguous()
    if store.dtype == torch.uint8:
        return ops.gather_tasks_resized_crop_flip_u8(table, c["geo"], lut, idx, params)
    return ops.gather_tasks_resized_crop_flip(table, c["geo"], idx, params)


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
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("C,Hs,Ws,th,tw", GEOMETRIES, ids=IDS)
def test_exemplar_rows_are_the_resizing_gather_bitwise(C, Hs, Ws, th, tw, byte):
    """Enlarging / 11 taps / mixed axes / the workload's shape / 17 taps / the plain-store width; 5 current rows, 3 ring rows,
    13 exemplar rows over hand-made windows and draws of the default spec.  The exemplar rows and their labels are the gather's
    over the store (one device body); everything else is a copy."""
    c = _case(C, Hs, Ws, th, tw, byte)
    got = _launch(c)
    _check_copy_and_ring(c, got)
    want, want_y = _gathered(c, got[0], got[1], got[5], c["gather"], c["params"])
    assert got[2].dtype == torch.float32 and bitwise_equal(got[2][B:], want) and torch.equal(got[3][B:], want_y)
    assert torch.equal(got[3][B:].cpu(), c["store_y"][c["gather"].long()])
    assert bool(torch.isfinite(got[2]).all()) and not bool((got[2] == -7.0).any())
    assert not torch.equal(got[2][B], got[2][B + 4])                # store row 9 under two windows


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("C,Hs,Ws,th,tw", [(3, 20, 20, 16, 16), (3, 13, 11, 8, 7), (1, 16, 16, 16, 16)],
                         ids=["20x20_to_16x16", "13x11_to_8x7", "no_freedom"])
def test_identity_windows_are_the_copying_assembly_bitwise(C, Hs, Ws, th, tw, byte):
    """h == th and w == tw: one tap of weight exactly 1 per axis, so x_mix, the labels and the store are those of
    clhip_rehearsal_assemble_crop_flip for (top, left, flip).  A -0.0 inside a window survives, an infinity beside it (taps of
    weight 0) takes no part."""
    c = dict(_case(C, Hs, Ws, th, tw, byte))
    mt, ml = Hs - th, Ws - tw
    p3 = torch.tensor([[0, 0, 0], [mt, ml, 1], [0, ml, 1], [mt, 0, 0], [mt, ml, 0], [mt // 2, min(1, ml), 0], [min(1, mt), ml // 2, 1],
                       [0, 0, 1], [mt, ml, 1], [0, 0, 0], [mt // 2, ml // 2, 1], [0, ml, 0], [mt, 0, 1]], dtype=torch.int32)
    c["store"] = c["store"].clone()
    if byte:                                                        # byte 7 means -0.0, byte 9 an infinity, and only where put
        c["lut"] = c["lut"].clone()
        c["lut"][:, 7], c["lut"][:, 9] = -0.0, float("inf")
        c["store"][(c["store"] == 7) | (c["store"] == 9)] = 8
        c["store"][9, 0, 0, 0] = 7                                  # row 9 is gathered at (0, 0): inside
        if mt and ml:
            c["store"][9, 0, th, tw] = 9                            # beside the window that starts at (0, 0)
    else:
        c["store"][9, 0, 0, 0] = -0.0
        if mt and ml:
            c["store"][9, 0, th, tw] = float("inf")
    assert GATHER[0] == 9 and p3[0].tolist() == [0, 0, 0]
    full = lambda v: torch.full((E,), v, dtype=torch.int32)         # noqa: E731
    c["params"] = torch.stack([p3[:, 0], p3[:, 1], full(th), full(tw), p3[:, 2]], 1).contiguous()
    got = _launch(c)
    c["params"] = p3
    want = _launch(c, crop=True)
    assert bitwise_equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool(torch.signbit(got[2][B, 0, 0, 0])) and float(got[2][B, 0, 0, 0]) == 0.0
    assert bool(torch.isfinite(got[2][B]).all())


def test_error_against_the_restatement_is_within_atens_own():
    """(3, 40, 33) -> 8 x 8, the fp32 store: the exemplar rows' distance from the fp64 restatement of the formula is at most MARGIN
    times that of ATen's fp32 CPU operator on the same rows."""
    c = _case(*GEOMETRIES[1])
    got = _launch(c)
    C, Hs, Ws, th, tw = c["geo"]
    store = got[0].cpu()
    want = ref.restate(store, c["gather"].long(), c["params"], th, tw)
    e_ref = float((ref.aten(store, c["gather"].long(), c["params"], th, tw).double() - want).abs().max())
    e_kernel = float((got[2][B:].cpu().double() - want).abs().max())
    print("exemplar rows %s: kernel error %.3g, ATen fp32 error %.3g" % (c["geo"], e_kernel, e_ref))
    assert e_ref > 0.0
    assert e_kernel <= MARGIN * e_ref


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_two_launches_are_bitwise_equal_and_an_unaligned_x_mix_takes_the_plain_path(byte):
    """tw % 4 == 0 and x_mix 4 bytes off a 16-byte boundary: no vector stores, the same values, nothing in front of the buffer."""
    c = _case(*GEOMETRIES[1], byte)
    a, b2, plain = _launch(c), _launch(c), _launch(c, offset=1)
    for other in (b2, plain):
        assert bitwise_equal(a[2], other[2]) and torch.equal(a[3], other[3]) and torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    assert plain[4].tolist() == [-7.0]
    _check_copy_and_ring(c, plain)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_launches_without_one_of_the_runs(byte):
    c = _case(3, 12, 10, 5, 7, byte)
    full = _launch(c)
    none = _launch(c, e=0)                                          # E == 0: no plan, no exemplar blocks
    _check_copy_and_ring(c, none)
    assert none[2].shape[0] == B and torch.equal(none[0], full[0])
    no_ring = _launch(c, ring=0)
    _check_copy_and_ring(c, no_ring, ring=0)
    assert torch.equal(no_ring[0].cpu(), c["store"]) and bitwise_equal(no_ring[2], full[2]) and torch.equal(no_ring[3], full[3])
    cc = dict(c, x=c["x"][:0])
    alone = _launch(cc, b=0, ring=0)                                # no current rows
    assert alone[2].shape[0] == E and bitwise_equal(alone[2], full[2][B:]) and torch.equal(alone[3], full[3][B:])


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_the_ring_update_alone_takes_no_x_mix_and_no_table(byte):
    """E = 0 and x_mix = NULL: GEM's fill_buffer.  The store rows and labels move, nothing else is touched; the byte entry needs
    no table."""
    c = _case(3, 12, 10, 5, 7, byte)
    got = _launch(c, e=0, x_mix=None, lut=None)
    assert got[2] is None and got[3] is None
    _check_copy_and_ring(c, got)
    assert not torch.equal(got[0].cpu(), c["store"])


BAD_GEO = (2, 20, 26, 2, 3)      # 17 lines are more than CLHIP_RESIZE_MAX_RATIO times 2 and fit the frame


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("bad", ["gather_row", "gather_row_negative", "top", "left", "h_zero", "w_past_the_frame", "flip", "h_over_ratio",
                                 "src_idx"])
def test_bad_rows_copy_nothing_and_get_label_minus_one(bad, byte):
    """One bad row between good ones: its x_mix row keeps the prefill and gets label -1 (src_idx: its store row keeps its frame
    and gets store label -1); every other row is what the launch of the good table gives."""
    ok = _case(*BAD_GEO, byte)
    c = copy.deepcopy(ok)
    k = 9                                                           # a drawn window
    c["params"][k] = torch.tensor([2, 3, 6, 8, 0], dtype=torch.int32)
    ok = copy.deepcopy(c)
    assert tuple(ok["params"].shape) == (E, 5)
    if bad == "gather_row":
        c["gather"][k] = STORE_ROWS
    elif bad == "gather_row_negative":
        c["gather"][k] = -1
    elif bad == "top":
        c["params"][k, 0] = -1
    elif bad == "left":
        c["params"][k, 1] = -1
    elif bad == "h_zero":
        c["params"][k, 2] = 0
    elif bad == "w_past_the_frame":
        c["params"][k, 3] = BAD_GEO[2] - 3 + 1
    elif bad == "flip":
        c["params"][k, 4] = 2
    elif bad == "h_over_ratio":
        c["params"][k, 2] = 8 * BAD_GEO[3] + 1
        assert 2 + 17 <= BAD_GEO[1]
    else:
        c["src_idx"][1] = SRC_ROWS
    got, want = [v.cpu() for v in _launch(c)[:4]], [v.cpu() for v in _launch(ok)[:4]]
    if bad == "src_idx":
        want[0][ROW0 + 1], want[1][ROW0 + 1] = c["store"][ROW0 + 1], -1
    else:
        want[2][B + k], want[3][B + k] = -7.0, -1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bitwise_equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert not bool((want[2][:B + k] == -7.0).any()) and not bool((want[2][B + k + 1:] == -7.0).any())


def test_argument_errors_come_before_any_launch():
    from clsurvey_amd import _lib, ops
    c = _case(3, 12, 10, 5, 7)
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm = torch.full((B + E, 3, 5, 7), -7.0, device=DEV)
    ym = torch.full((B + E,), 99, dtype=torch.int64, device=DEV)
    store0 = d["store"].clone()

    def call(geo=c["geo"], b=B, row0=ROW0, ring=RING, params=d["params"]):
        ops.rehearsal_assemble_resized_crop_flip(geo, d["x"], d["y"], b, d["src"], d["src_idx"], d["store"], d["store_y"], row0, ring,
                                                 d["gather"], params, xm, ym)
    for kw in (dict(row0=-1), dict(row0=STORE_ROWS - RING + 1), dict(b=-1, ring=0)):
        with pytest.raises(_lib.ClhipError, match="CLHIP_EINVAL"):
            call(**kw)
    for geo in ((3, 12, 10, 0, 7), (3, 12, 10, 5, 0)):
        with pytest.raises(_lib.ClhipError, match="CLHIP_EINVAL"):
            call(geo=geo)
    with pytest.raises(AssertionError):                             # the crop entry's table has another shape
        call(params=d["params"][:, :3].contiguous())
    with pytest.raises(AssertionError):
        call(params=d["params"].long())
    torch.cuda.synchronize()
    assert bool((xm == -7.0).all()) and bool((ym == 99).all()) and torch.equal(d["store"], store0)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_a_frame_whose_plan_does_not_fit_is_enotsup_only_with_exemplars(byte):
    """1000 -> 125: the band of one output line does not fit the LDS.  The plan is made on the host for the frame, so a one-frame
    store suffices; with E == 0 no plan is needed and the copy and ring rows are served."""
    from clsurvey_amd import _lib, ops
    geo = (1, 1000, 1000, 125, 125)
    dt = torch.uint8 if byte else torch.float32
    store, src = torch.zeros((1,) + geo[:3], dtype=dt, device=DEV), torch.ones((1,) + geo[:3], dtype=dt, device=DEV)
    store_y, y = torch.tensor([5], device=DEV), torch.tensor([3], device=DEV)
    x = torch.randn((1, 1, 125, 125), device=DEV)
    xm, ym = torch.full((2, 1, 125, 125), -7.0, device=DEV), torch.full((2,), 99, dtype=torch.int64, device=DEV)
    gather = torch.tensor([0], dtype=torch.int32, device=DEV)
    params = torch.tensor([[0, 0, 1000, 1000, 0]], dtype=torch.int32, device=DEV)
    if byte:
        lut = torch.randn((1, 256), device=DEV)
        entry = functools.partial(ops.rehearsal_assemble_resized_crop_flip_u8, geo, lut)
    else:
        entry = functools.partial(ops.rehearsal_assemble_resized_crop_flip, geo)
    idx = torch.tensor([0], device=DEV)
    with pytest.raises(_lib.ClhipError, match="CLHIP_ENOTSUP"):
        entry(x, y, 1, src, idx, store, store_y, 0, 1, gather, params, xm, ym)
    torch.cuda.synchronize()
    assert bool((xm == -7.0).all()) and int(store.sum()) == 0 and store_y.tolist() == [5]
    entry(x, y, 1, src, idx, store, store_y, 0, 1, None, None, xm, ym)
    torch.cuda.synchronize()
    assert bitwise_equal(xm[0], x[0]) and bool((xm[1] == -7.0).all()) and ym.tolist() == [3, 99]
    assert torch.equal(store, src) and store_y.tolist() == [3]


# ---------------------------------------------------------------------------------------------- the wrappers
HW, MARG, NCLS, N_TRAIN, BATCH, N_MEM = 16, 4, 4, 24, 8, 5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _net():
    """As test_gpu_u8_exemplar._net, for 16 x 16 inputs."""
    from clsurvey_amd.models import VGGSlim
    return VGGSlim(cfg=[8, "M", 16, "M"], num_classes=NCLS, classifier_inputdim=16 * 4 * 4, classifier_dim1=32, classifier_dim2=32,
                   dropout=True, batch_norm=False)


def _resized(extents=None, **kw):
    from clsurvey_amd.data import RandomResizedCropFlip
    return RandomResizedCropFlip((HW, HW), extents=extents, **kw)


@functools.lru_cache(maxsize=None)
def _tasks():
    """Two byte tasks of 24 frames 3 x 20 x 20 under the default resized spec, each frame with a valid extent of its own, and
    their decoded twins, on the device."""
    from clsurvey_amd.data import ByteTaskDataset
    gen = torch.Generator().manual_seed(21)
    out = []
    for _ in range(2):
        y = torch.randint(0, NCLS, (N_TRAIN,), generator=gen)
        x = (torch.randn((N_TRAIN, 3, HW + MARG, HW + MARG), generator=gen) * 40 + 128 + (y[:, None, None, None] - 1.5) * 25)
        ext = torch.randint(HW, HW + MARG + 1, (N_TRAIN, 2), generator=gen)
        byte = ByteTaskDataset(x.round().clamp(0, 255).to(torch.uint8).to(DEV), y.to(DEV), [str(k) for k in range(NCLS)], MEAN, STD,
                               transform=_resized(ext))
        out.append((byte, byte.decoded()))
    return out


@functools.lru_cache(maxsize=None)
def _square_tasks():
    """Two float tasks of 24 frames of the net's input size, without a transform: the tests attach theirs."""
    gen = torch.Generator().manual_seed(22)
    out = []
    for _ in range(2):
        y = torch.randint(0, NCLS, (N_TRAIN,), generator=gen)
        x = torch.randn((N_TRAIN, 3, HW, HW), generator=gen) + (y[:, None, None, None] - 1.5) * 0.5
        out.append((x.to(DEV), y.to(DEV)))
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


def _same_traces(ta, tb, same_draws=True):
    assert len(ta) == len(tb) == 6
    for (la, ha, pa, ga, da), (lb, hb, pb, gb, db) in zip(ta, tb):
        assert bitwise_equal(la.reshape(1), lb.reshape(1)) and bool(torch.isfinite(la).all())
        if torch.is_tensor(ha):
            assert torch.equal(ha, hb)
        for p, q in zip(pa, pb):
            assert bitwise_equal(p, q)
        assert ga == gb and (da is None) == (db is None)
        if same_draws and da is not None:
            assert torch.equal(da, db)
    assert any(not torch.equal(p, q) for p, q in zip(ta[0][2], ta[-1][2]))          # the steps did train


def test_a_step_replays_the_draws_of_its_seed_through_the_gather():
    """After RehearsalNet.observe_FT: last_exemplar_params is draw_resized_crop_flip over store_ext[last_gather] from the seed the
    plan handed out, and x_mix[B:N] is bitwise the resizing gather over the store for those rows and windows."""
    from clsurvey_amd.data import DeviceLoader, draw_resized_crop_flip
    tasks = [dec for _, dec in _tasks()]
    w = _wrapper("partial", _resized(), HW + MARG)
    _run(w, tasks[:1], steps=3)
    w.init_setup(lr=0.02, weight_decay=1e-4, n_append=3, chunk_size=2)
    seen, orig = [], w.plan

    def plan(t, seeds=None):
        out = orig(t, seeds)
        seen[:] = list(seeds)
        return out
    w.plan = plan
    torch.manual_seed(13)
    random.seed(13)
    loader = DeviceLoader(tasks[1], BATCH, True, DEV)
    x, y = next(iter(loader))
    _step(w, loader, x, 1, y)
    rows, params = w.last_gather, w.last_exemplar_params
    assert len(rows) == 3 and all(0 <= r < N_MEM for r in rows) and tuple(params.shape) == (3, 5) and params.dtype == torch.int32
    ext = w.store_ext[torch.tensor(rows)]
    assert int(ext.min()) >= HW and int(ext.max()) <= HW + MARG
    want = draw_resized_crop_flip(3, _resized(ext), (HW + MARG, HW + MARG), torch.Generator().manual_seed(seen[-1]))
    assert torch.equal(params, want)
    p = params.long()
    assert bool((p[:, 0] + p[:, 2] <= ext[:, 0]).all()) and bool((p[:, 1] + p[:, 3] <= ext[:, 1]).all())
    c = dict(geo=w.geometry)
    gx, gy = _gathered(c, w.store_x, w.store_y, None, torch.tensor(rows), params)
    assert bitwise_equal(w.x_mix[BATCH:BATCH + 3], gx) and torch.equal(w.y_mix[BATCH:BATCH + 3], gy)
    assert bitwise_equal(w.x_mix[:BATCH], x) and torch.equal(w.y_mix[:BATCH], y)


@pytest.mark.parametrize("kind,segmented", [("partial", False), ("partial", True), ("full", False), ("full", True), ("gem", False)],
                         ids=["R-PM-fused", "R-PM-segmented", "R-FM-fused", "R-FM-segmented", "GEM"])
def test_a_spec_without_freedom_is_the_crop_run(kind, segmented):
    """scale = ratio = (1, 1), p = 0 on frames of the input size: every window is the whole frame and every tap has weight 1, so
    losses, hits, parameters and the store are bitwise those of the RandomCropFlip(p = 0) frame-mode run."""
    from clsurvey_amd.data import RandomCropFlip, TensorTaskDataset
    classes = [str(k) for k in range(NCLS)]
    runs = []
    for spec in (_resized(scale=(1, 1), ratio=(1, 1), p=0.0), RandomCropFlip((HW, HW), 0.0)):
        dsets = [TensorTaskDataset(x, y, classes, transform=spec) for x, y in _square_tasks()]
        w = _wrapper(kind, spec, HW, segmented=segmented)
        runs.append((w, _run(w, dsets)))
    (a, ta), (b, tb) = runs
    assert type(a.exemplar_transform).__name__ == "RandomResizedCropFlip" and type(b.exemplar_transform).__name__ == "RandomCropFlip"
    _same_traces(ta, tb, same_draws=False)
    for u, v in zip(_store(a), _store(b)):
        assert torch.equal(u, v)
    if kind != "gem":
        assert a.last_path == b.last_path == ("segmented" if segmented else "fused")
        assert a.last_exemplar_params.tolist() == [[0, 0, HW, HW, 0]] * 3 and b.last_exemplar_params.tolist() == [[0, 0, 0]] * 3
        assert bitwise_equal(a.x_mix[:BATCH + 3], b.x_mix[:BATCH + 3]) and torch.equal(a.y_mix[:BATCH + 3], b.y_mix[:BATCH + 3])


@pytest.mark.parametrize("kind", ["partial", "gem"])
def test_a_byte_store_run_is_the_fp32_run_on_the_decoded_split(kind):
    from clsurvey_amd.data import norm_lut
    tasks = _tasks()
    a = _wrapper(kind, _resized(), HW + MARG, byte=True)
    ta = _run(a, [byte for byte, _ in tasks])
    b = _wrapper(kind, _resized(), HW + MARG)
    tb = _run(b, [dec for _, dec in tasks])
    assert a.frame_norm is not None and b.frame_norm is None and a.store_dtype == torch.uint8
    _same_traces(ta, tb)
    (bx, by, bext), (fx, fy, fext) = _store(a), _store(b)
    lut = norm_lut(*a.frame_norm)
    dec = torch.stack([lut[ch][bx.cpu()[:, ch].long()] for ch in range(3)], 1)
    assert bx.dtype == torch.uint8 and int(bx.max()) > 0 and bitwise_equal(dec, fx)
    assert torch.equal(by, fy) and torch.equal(bext, fext) and int(bext.min()) < HW + MARG
    if kind != "gem":
        assert tuple(a.last_exemplar_params.shape) == (3, 5) and len({tuple(r[2:4]) for r in a.last_exemplar_params.tolist()}) > 1
        assert bitwise_equal(a.x_mix[:BATCH + 3], b.x_mix[:BATCH + 3]) and torch.equal(a.y_mix[:BATCH + 3], b.y_mix[:BATCH + 3])


@pytest.mark.parametrize("kind", ["partial", "gem"])
def test_pickle_round_trip_gives_the_same_next_step(kind):
    from clsurvey_amd.data import DeviceLoader, RandomResizedCropFlip
    tasks = [dec for _, dec in _tasks()]
    spec = _resized(scale=(0.3, 0.9), ratio=(0.6, 1.5), p=0.25)
    w = _wrapper(kind, spec, HW + MARG)
    _run(w, tasks, steps=2)
    buf = io.BytesIO()
    torch.save(w, buf)
    buf.seek(0)
    w2 = torch.load(buf, weights_only=False)
    t = w2.exemplar_transform
    assert isinstance(t, RandomResizedCropFlip) and t.extents is None
    assert (t.size, t.scale, t.ratio, t.p) == ((HW, HW), (0.3, 0.9), (0.6, 1.5), 0.25) and w2.params_width == 5
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


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_gems_memory_loader_carries_the_spec_and_the_memorys_extents(byte):
    from clsurvey_amd.data import ByteTaskDataset, RandomResizedCropFlip
    tasks = _tasks()
    spec = _resized(scale=(0.3, 0.9), ratio=(0.6, 1.5), p=0.25)
    w = _wrapper("gem", spec, HW + MARG, byte=byte)
    _run(w, [d[0 if byte else 1] for d in tasks], steps=1)
    loader = w._memory_loader(0)
    t = loader.transform
    assert isinstance(t, RandomResizedCropFlip) and (t.size, t.scale, t.ratio, t.p) == ((HW, HW), (0.3, 0.9), (0.6, 1.5), 0.25)
    assert torch.equal(t.extents, w.memory_ext[0]) and int(t.extents.min()) < HW + MARG
    assert isinstance(loader.dataset, ByteTaskDataset) == byte and loader._resized
    x, y = next(iter(loader))
    assert tuple(x.shape) == (N_MEM, 3, HW, HW) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())


# ---------------------------------------------------------------------------------------------- gem_main.main
def _seeds(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _dicts(root, byte):
    """The resized files of two synthetic tasks (frames 3 x 36 x 36 -> 32 x 32), loaded to the device."""
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="rz", u8_frames=byte, rnd_resized=4)
    return [load_task_datasets(ds.get_task_dataset_path(str(t), rnd_transform=True), DEV) for t in (1, 2)]


def _base_model(path):
    from clsurvey_amd import models
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), path)
    return path


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_rehearsal_partial_mem_entry_builds_then_loads_with_the_switch(tmp_path, byte):
    from clsurvey_amd.data import RandomResizedCropFlip
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dicts = _dicts(root, byte)
    assert all(isinstance(d["train"].transform, RandomResizedCropFlip) for d in dicts)
    prev = _base_model(os.path.join(root, "prev.pth.tar"))
    common = dict(n_outputs=8, method="baseline_rehearsal_partial_mem", n_memories=6, n_tasks=2, postprocess=False, n_epochs=1,
                  batch_size=16, lr=1e-2, exemplar_resized=True, **({"exemplar_dtype": "uint8"} if byte else {}))
    dt = torch.uint8 if byte else torch.float32
    _seeds(11)
    m1, acc1 = gem_main.main(dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0],
                                  is_scratch_model=True, save_path=os.path.join(root, "t1")), [4, 4], device=DEV)
    assert isinstance(m1.exemplar_transform, RandomResizedCropFlip) and m1.exemplar_transform.size == (32, 32)
    assert m1.store_x.dtype == dt and tuple(m1.store_x.shape) == (12, 3, 36, 36) and m1.filled == [6, 0] and 0.0 <= acc1 <= 1.0
    assert float(m1.store_x[:6].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and float(m1.store_x[6:].float().abs().sum()) == 0
    saved = os.path.join(root, "t1", "best_model.pth.tar")
    m2, acc2 = gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=saved, dataset_path=dicts[1],
                                  is_scratch_model=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert isinstance(m2.exemplar_transform, RandomResizedCropFlip) and m2.store_x.dtype == dt
    assert m2.filled == [6, 6] and m2.last_path == "fused" and len(m2.last_gather) > 0 and 0.0 <= acc2 <= 1.0
    assert tuple(m2.last_exemplar_params.shape) == (len(m2.last_gather), 5)
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_gem_entry_builds_then_loads_with_the_switch(tmp_path, byte):
    from clsurvey_amd.data import RandomResizedCropFlip
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dicts = _dicts(root, byte)
    prev = _base_model(os.path.join(root, "SI", "prev.pth.tar"))
    common = dict(n_outputs=8, method="gem", n_memories=6, n_tasks=2, n_epochs=1, batch_size=16, lr=1e-2, memory_strength=0.5,
                  exemplar_resized=True, **({"exemplar_dtype": "uint8"} if byte else {}))
    dt = torch.uint8 if byte else torch.float32
    _seeds(12)
    wrapped = os.path.join(root, "t1", "best_model.pth.tar")
    gem_main.main(dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0], is_scratch_model=True,
                       postprocess=True, save_path=wrapped), [4, 4], device=DEV)
    w = torch.load(wrapped, weights_only=False)
    assert isinstance(w.exemplar_transform, RandomResizedCropFlip) and (w.frame_norm is not None) == byte
    assert w.memory_x.dtype == dt and tuple(w.memory_x.shape) == (2, 6, 3, 36, 36)
    assert float(w.memory_x[0].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and float(w.memory_x[1].float().abs().sum()) == 0
    m2, acc2 = gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=wrapped, dataset_path=dicts[1],
                                  is_scratch_model=False, postprocess=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert m2.memory_x.dtype == dt and m2.observed_tasks == [0, 1] and 0.0 <= acc2 <= 1.0
    assert float(m2.memory_x[1].float().abs().sum(dim=(1, 2, 3)).min()) > 0 and torch.equal(m2.memory_x[0], w.memory_x[0])
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())


# ---------------------------------------------------------------------------------------------- through the driver
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_rehearsal_partial_mem_through_the_driver_on_resized_tasks(tmp_path, byte):
    from clsurvey_amd import models
    from clsurvey_amd.data import RandomResizedCropFlip
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
            "--results_root", root, "--synthetic", "2,4,160,40,40,32", "--rnd_resized", "4", "--resized_exemplars",
            "--method_name", "finetuning_rehearsal_partial_mem", "--test", "--mem_per_task", "24"]
    if byte:
        argv += ["--u8_frames", "--u8_exemplars"]
    out = driver.main(argv)
    res = out["results"]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("R-PM on resized tasks:", accs)
    assert sorted(res) == [0, 1] and len(accs) > 0 and all(a == a and 0.0 <= a <= 100.0 for a in accs)
    for k, path in enumerate(out["model_paths"], start=1):
        w = torch.load(path, weights_only=False)
        assert isinstance(w.exemplar_transform, RandomResizedCropFlip) and w.exemplar_transform.size == (32, 32)
        assert w.store_x.dtype == (torch.uint8 if byte else torch.float32) and tuple(w.store_x.shape) == (48, 3, 36, 36)
        assert w.filled[:k] == [24] * k and (w.frame_norm is not None) == byte
        assert float(w.store_x[:24 * k].float().abs().sum(dim=(1, 2, 3)).min()) > 0
