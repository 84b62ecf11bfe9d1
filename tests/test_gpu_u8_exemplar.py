"""The byte exemplar store on the GPU: clhip_rehearsal_assemble_crop_flip_u8 against the fp32 entry run on the decoded frames and
against a torch restatement by indexing; RehearsalNet (partial / full memory, fused / segmented) and GemNet with a byte store
against their fp32 frame-mode runs on `split.decoded()`; the pickle; gem_main.main and the driver with the switch.  Every
comparison of values is torch.equal on the int32 view (or on bytes): no tolerance."""
import copy
import functools
import io
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, RING, ROW0, STORE_ROWS, SRC_ROWS = 5, 3, 4, 12, 9
GATHER = [9, 0, 3, 11, 9, 1, 8]                                   # E = 7, store row 9 twice; none of the ring rows 4..6
SRC_IDX = [7, 0, 3]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _decode(x, lut):
    """The meaning of byte frames [n][C][H][W]: lut[c][x]."""
    return torch.stack([lut[c][x[:, c].long()] for c in range(x.shape[1])], 1)


def restate(frames, rows, params, th, tw):
    """torchvision's crop, then hflip, of frames[rows[e]] with params[e] = (top, left, flip), on the CPU."""
    out = [frames[g, :, top:top + th, left:left + tw] for g, (top, left, _) in zip(rows, params.tolist())]
    return torch.stack([v.flip(-1) if flip else v for v, (_, _, flip) in zip(out, params.tolist())])


def _params(Hs, Ws, th, tw):
    """Offsets 0 and the maximum in both axes, both flip values, two rows for store row 9."""
    mt, ml = Hs - th, Ws - tw
    return torch.tensor([[0, 0, 0], [mt, ml, 1], [0, ml, 1], [mt, 0, 0], [mt // 2, min(1, ml), 1], [min(1, mt), ml // 2, 0],
                         [mt, min(3, ml), 1]], dtype=torch.int32)


def _random_lut(C, gen):
    """fp32 [C][256] of random values with +0.0, -0.0, a denormal and an infinity among them: a copy keeps every bit."""
    lut = torch.randn((C, 256), generator=gen)
    lut[:, 0], lut[:, 1], lut[:, 255] = 0.0, -0.0, float("inf")
    lut[:, 2] = torch.tensor([1], dtype=torch.int32).view(torch.float32)          # the smallest denormal
    return lut


@functools.lru_cache(maxsize=None)
def _case(C, Hs, Ws, th, tw, seed):
    """Made once per geometry and never written to (the launches work on device copies)."""
    gen = torch.Generator().manual_seed(seed)
    store = torch.randint(0, 256, (STORE_ROWS, C, Hs, Ws), generator=gen, dtype=torch.uint8)
    n = min(256, C * Hs * Ws)
    store[9].view(-1)[:n] = torch.arange(n, dtype=torch.uint8)     # (a frame of 256 bytes or more: every byte value in a gathered row)
    return dict(geo=(C, Hs, Ws, th, tw), lut=_random_lut(C, gen),
                x=torch.randn((B, C, th, tw), generator=gen), y=torch.randint(0, 20, (B,), generator=gen),
                src=torch.randint(0, 256, (SRC_ROWS, C, Hs, Ws), generator=gen, dtype=torch.uint8), src_idx=torch.tensor(SRC_IDX),
                store=store, store_y=torch.randint(0, 20, (STORE_ROWS,), generator=gen),
                gather=torch.tensor(GATHER, dtype=torch.int32), params=_params(Hs, Ws, th, tw))


def _launch(c, b=B, ring=RING, e=len(GATHER), x_mix="new", offset=0, store_offset=0, fp32=False):
    """Runs the byte entry (fp32: the fp32 entry on the decoded frames) on device copies of case c; returns the CPU (store,
    store_y, x_mix, y_mix, guard floats in front of x_mix, guard bytes in front of the store)."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = c["geo"]
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    if fp32:
        store, src = _decode(c["store"], c["lut"]).to(DEV), _decode(c["src"], c["lut"]).to(DEV)
        sbuf = None
    else:
        sbuf = torch.full((store_offset + c["store"].numel(),), 201, dtype=torch.uint8, device=DEV)
        store = sbuf[store_offset:].view(c["store"].shape).copy_(d["store"])
        assert store.data_ptr() % 16 == store_offset
        src = d["src"]
    xm = ym = buf = None
    if x_mix is not None:
        buf = torch.full((offset + (b + e) * C * th * tw,), -7.0, device=DEV)
        xm = buf[offset:]
        ym = torch.full((b + e,), 99, dtype=torch.int64, device=DEV)
    args = (d["x"][:b].contiguous(), d["y"], b, src, d["src_idx"], store, d["store_y"], ROW0, ring, d["gather"][:e] if e else None,
            d["params"][:e] if e else None, xm, ym)
    if fp32:
        ops.rehearsal_assemble_crop_flip(c["geo"], *args)
    else:
        ops.rehearsal_assemble_crop_flip_u8(c["geo"], d["lut"], *args)
    torch.cuda.synchronize()
    return (store.cpu(), d["store_y"].cpu(), None if xm is None else xm.cpu().view(b + e, C, th, tw),
            None if ym is None else ym.cpu(), None if buf is None else buf[:offset].cpu(), None if sbuf is None else sbuf[:store_offset].cpu())


def _expect(c, b=B, ring=RING, e=len(GATHER)):
    """By indexing on the CPU: (byte store, store labels, x_mix, y_mix)."""
    C, Hs, Ws, th, tw = c["geo"]
    store, store_y = c["store"].clone(), c["store_y"].clone()
    store[ROW0:ROW0 + ring] = c["src"].index_select(0, c["src_idx"][:ring])
    store_y[ROW0:ROW0 + ring] = c["y"][:ring]
    rows = c["gather"][:e].long()
    ex = restate(_decode(store, c["lut"]), rows.tolist(), c["params"][:e], th, tw) if e else torch.zeros((0, C, th, tw))
    return store, store_y, torch.cat([c["x"][:b], ex]), torch.cat([c["y"][:b], store_y.index_select(0, rows)])


def _check(got, want, untouched_from=None):
    assert got[0].dtype == torch.uint8 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if want[2] is not None and got[2] is not None:
        assert got[2].dtype == torch.float32 and torch.equal(_bits(got[2]), _bits(want[2])) and torch.equal(got[3], want[3])
    if untouched_from is not None:
        keep = [r for r in range(STORE_ROWS) if not ROW0 <= r < ROW0 + RING]
        assert torch.equal(got[0][keep], untouched_from["store"][keep]) and torch.equal(got[1][keep], untouched_from["store_y"][keep])


def _two_segments(odd):
    """A one-channel frame just over one block's copy segment: two segments, the second one short.  224 lines: a multiple of 16
    bytes whatever the width (the 16-byte path); 223 lines of an odd width: an odd size (the byte path)."""
    from clsurvey_amd import ops
    Hs = 223 if odd else 224
    Ws = ops.ASSEMBLE_SEG_BYTES // Hs + 1
    if odd and Ws % 2 == 0:
        Ws += 1
    assert ops.ASSEMBLE_SEG_BYTES < Hs * Ws < ops.ASSEMBLE_SEG_BYTES + 2 * Hs + 1
    assert (Hs * Ws) % 2 == 1 if odd else (Hs * Ws) % 16 == 0
    return (1, Hs, Ws, 8, 8)


GEOMETRIES = [(1, 9, 11, 5, 6), (3, 13, 13, 8, 8), (3, 16, 16, 8, 8), (2, 8, 8, 8, 8), (3, 72, 72, 64, 64), "two_segments_16B",
              "two_segments_bytes"]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g if isinstance(g, str) else "%dx%dx%d_to_%dx%d" % g for g in GEOMETRIES])
def test_kernel_copies_bytes_and_decodes_the_cropped_gather(geo):
    """Odd everything (byte paths) / a 507-byte frame: frames at odd addresses under float4 stores and the tested dword load / a
    768-byte frame on the 16-byte ring path / no freedom / the product shape / a frame of two copy segments on either path.
    The stored bytes are the source bytes, the other store rows keep theirs, and x_mix / labels_mix are bitwise both the fp32
    entry on the decoded frames and the restatement by indexing."""
    if isinstance(geo, str):
        geo = _two_segments(geo.endswith("bytes"))
    c = _case(*geo, seed=sum(geo))
    got, want, ref = _launch(c), _expect(c), _launch(c, fp32=True)
    _check(got, want, untouched_from=c)
    assert torch.equal(got[0][ROW0:ROW0 + RING], c["src"][SRC_IDX])
    assert torch.equal(_bits(got[2]), _bits(ref[2])) and torch.equal(got[3], ref[3]) and torch.equal(got[1], ref[1])
    assert torch.equal(_bits(_decode(got[0], c["lut"])), _bits(ref[0]))
    if geo[1] > geo[3] and geo[2] > geo[4]:
        assert not torch.equal(got[2][B], got[2][B + 4])           # store row 9 under two parameter rows


def test_unaligned_tensors_take_the_plain_paths():
    """A 768-byte frame, tw % 4 == 0: the store one byte off a 16-byte boundary (byte ring copies, crop lines at odd addresses)
    and x_mix 4 bytes off (no vector stores).  Same bytes; the byte and the float in front are untouched."""
    c = _case(3, 16, 16, 8, 8, seed=4)
    got, want = _launch(c, offset=1, store_offset=1), _expect(c)
    _check(got, want, untouched_from=c)
    assert got[4].tolist() == [-7.0] and got[5].tolist() == [201]
    got = _launch(c, store_offset=1)                               # vector stores, unaligned byte lines
    _check(got, want, untouched_from=c)


def test_kernel_ring_update_alone_takes_no_x_mix_and_no_table():
    """E = 0 and x_mix = NULL: GEM's fill_buffer.  The store rows and labels move, nothing else is touched; lut may be None."""
    from clsurvey_amd import ops
    c = _case(3, 13, 13, 8, 8, seed=2)
    got = _launch(c, e=0, x_mix=None)
    want = _expect(c, e=0)
    assert got[2] is None and got[3] is None
    _check(got, want, untouched_from=c)
    assert not torch.equal(got[0], c["store"])
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    ops.rehearsal_assemble_crop_flip_u8(c["geo"], None, None, d["y"], B, d["src"], d["src_idx"], d["store"], d["store_y"], ROW0, RING,
                                        None, None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(d["store"].cpu(), want[0]) and torch.equal(d["store_y"].cpu(), want[1])


def test_kernel_without_ring_rows():
    c = _case(3, 13, 13, 8, 8, seed=3)
    got, want = _launch(c, ring=0), _expect(c, ring=0)
    _check(got, want)
    assert torch.equal(got[0], c["store"])


def test_kernel_without_current_rows():
    c = dict(_case(3, 13, 13, 8, 8, seed=1))
    c["x"] = c["x"][:0]
    got, want = _launch(c, b=0, ring=0), _expect(c, b=0, ring=0)
    _check(got, want)
    assert got[2].shape[0] == len(GATHER)


@pytest.mark.parametrize("bad", ["gather_row", "top", "left", "flip", "src_idx"])
def test_bad_rows_copy_nothing_and_get_label_minus_one(bad):
    """A gather row equal to store_rows, top / left one past their range, flip = 2: that row of x_mix keeps its prefill and gets
    label -1.  src_idx = src_rows: that store row keeps its bytes and gets store label -1.  Every other row is exact."""
    geo = (3, 13, 13, 8, 8)
    ok = _case(*geo, seed=5)
    c = copy.deepcopy(ok)
    if bad == "gather_row":
        c["gather"][2] = STORE_ROWS
    elif bad == "top":
        c["params"][2, 0] = geo[1] - geo[3] + 1
    elif bad == "left":
        c["params"][2, 1] = geo[2] - geo[4] + 1
    elif bad == "flip":
        c["params"][2, 2] = 2
    else:
        c["src_idx"][1] = SRC_ROWS
    store, store_y, xm, ym, _, _ = _launch(c)
    w_store, w_sy, w_xm, w_ym = _expect(ok)
    if bad == "src_idx":
        w_store[ROW0 + 1], w_sy[ROW0 + 1] = c["store"][ROW0 + 1], -1
    else:
        w_xm[B + 2], w_ym[B + 2] = -7.0, -1
    assert torch.equal(store, w_store) and torch.equal(store_y, w_sy) and torch.equal(_bits(xm), _bits(w_xm)) and torch.equal(ym, w_ym)


def test_the_wrapper_checks_dtypes_and_the_table():
    from clsurvey_amd import ops
    c = _case(3, 13, 13, 8, 8, seed=6)
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm, ym = torch.empty((B + 7, 3, 8, 8), device=DEV), torch.empty((B + 7,), dtype=torch.int64, device=DEV)

    def call(lut=d["lut"], src=d["src"], store=d["store"]):
        ops.rehearsal_assemble_crop_flip_u8(c["geo"], lut, d["x"], d["y"], B, src, d["src_idx"], store, d["store_y"], ROW0, RING,
                                            d["gather"], d["params"], xm, ym)
    call()
    for kw in (dict(store=d["store"].float()), dict(src=d["src"].float()), dict(lut=d["lut"][:2].contiguous()), dict(lut=d["lut"].double())):
        with pytest.raises(AssertionError):
            call(**kw)
    with pytest.raises(AssertionError):
        call(lut=None)


# ---------------------------------------------------------------------------------------------- the wrappers
HW, MARGIN, NCLS, N_TRAIN, BATCH, N_MEM = 32, 4, 4, 24, 8, 5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _net():
    from clsurvey_amd.models import VGGSlim
    return VGGSlim(cfg=[8, "M", 16, "M"], num_classes=NCLS, classifier_inputdim=16 * 8 * 8, classifier_dim1=32, classifier_dim2=32,
                   dropout=True, batch_norm=False)


@functools.lru_cache(maxsize=None)
def _tasks():
    """Two byte tasks of 24 frames 3 x 36 x 36, each with a valid extent of its own, and their decoded twins, on the device."""
    from clsurvey_amd.data import ByteTaskDataset, RandomCropFlip
    gen = torch.Generator().manual_seed(21)
    out = []
    for _ in range(2):
        y = torch.randint(0, NCLS, (N_TRAIN,), generator=gen)
        x = (torch.randn((N_TRAIN, 3, HW + MARGIN, HW + MARGIN), generator=gen) * 40 + 128 + (y[:, None, None, None] - 1.5) * 25)
        ext = torch.randint(HW, HW + MARGIN + 1, (N_TRAIN, 2), generator=gen)
        byte = ByteTaskDataset(x.round().clamp(0, 255).to(torch.uint8).to(DEV), y.to(DEV), [str(k) for k in range(NCLS)], MEAN, STD,
                               transform=RandomCropFlip((HW, HW), 0.5, ext))
        out.append((byte, byte.decoded()))
    return out


def _wrapper(kind, byte, segmented=False):
    from clsurvey_amd.data import RandomCropFlip
    from clsurvey_amd.methods.gem import GemNet, extend_head
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    torch.manual_seed(5)
    kw = dict(exemplar_transform=RandomCropFlip((HW, HW), 0.5), frame_shape=(3, HW + MARGIN, HW + MARGIN))
    if byte:
        kw["frame_norm"] = (MEAN, STD)
    if kind == "gem":
        w = GemNet(extend_head(_net(), 2 * NCLS), 2 * NCLS, 2, [NCLS] * 2, N_MEM, lr=0.02, memory_strength=0.5, batch_size=BATCH,
                   in_shape=(3, HW, HW), device=DEV, **kw)
    else:
        w = RehearsalNet(replace_head(_net(), 2 * NCLS), 2 * NCLS, 2, [NCLS] * 2, N_MEM, 0.02, 1e-4, kind == "full", BATCH + 3,
                         (3, HW, HW), DEV, **kw)
        w.force_segmented = segmented
    return w


def _store(w):
    from clsurvey_amd.methods.gem import GemNet
    if isinstance(w, GemNet):
        return w.memory_x.view((-1,) + w.frame_shape), w.memory_labels.view(-1), w.memory_ext.view(-1, 2)
    return w.store_x, w.store_y, w.store_ext


def _run(w, dsets, steps=3):
    """Two tasks, `steps` steps each, from a fixed RNG state.  Returns per step (loss, parameters, gather rows, exemplar draws)."""
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.exemplar import batch_source
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
            src = batch_source(loader)
            out = w.observe(x, t, y, source=src) if isinstance(w, GemNet) else w.observe_FT(x, t, y, source=src)
            trace.append((out[0].clone(), [p.detach().clone() for p in w.parameters()], copy.copy(w.__dict__.get("last_gather")),
                          w.__dict__.get("last_exemplar_params")))
    torch.cuda.synchronize()
    return trace


def _same_traces(ta, tb):
    assert len(ta) == len(tb) == 6
    for (la, pa, ga, da), (lb, pb, gb, db) in zip(ta, tb):
        assert torch.equal(_bits(la.reshape(1)), _bits(lb.reshape(1))) and bool(torch.isfinite(la).all())
        for p, q in zip(pa, pb):
            assert torch.equal(_bits(p), _bits(q))
        assert ga == gb and (da is None) == (db is None) and (da is None or torch.equal(da, db))
    assert any(not torch.equal(p, q) for p, q in zip(ta[0][1], ta[-1][1]))          # the steps did train


def _same_stores(byte, flt):
    from clsurvey_amd.data import norm_lut
    (bx, by, bext), (fx, fy, fext) = _store(byte), _store(flt)
    assert bx.dtype == torch.uint8 and fx.dtype == torch.float32 and bx.shape == fx.shape and int(bx.max()) > 0
    lut = norm_lut(*byte.frame_norm)
    assert torch.equal(_bits(_decode(bx.cpu(), lut)), _bits(fx.cpu()))
    assert torch.equal(by, fy) and torch.equal(bext, fext) and int(bext.min()) < HW + MARGIN


@pytest.mark.parametrize("kind,segmented", [("partial", False), ("partial", True), ("full", False), ("full", True), ("gem", False)],
                         ids=["R-PM-fused", "R-PM-segmented", "R-FM-fused", "R-FM-segmented", "GEM"])
def test_a_byte_store_run_is_the_fp32_frame_mode_run_on_the_decoded_split(kind, segmented):
    tasks = _tasks()
    a = _wrapper(kind, True, segmented)
    ta = _run(a, [byte for byte, _ in tasks])
    b = _wrapper(kind, False, segmented)
    tb = _run(b, [dec for _, dec in tasks])
    assert a.frame_norm is not None and b.frame_norm is None and a.lut.is_cuda and tuple(a.lut.shape) == (3, 256)
    _same_traces(ta, tb)
    _same_stores(a, b)
    if kind != "gem":
        assert a.last_path == b.last_path == ("segmented" if segmented else "fused")
        assert len(a.last_gather) == 3 and int(a.last_exemplar_params[:, :2].max()) <= MARGIN
        assert torch.equal(_bits(a.x_mix[:BATCH + 3]), _bits(b.x_mix[:BATCH + 3])) and torch.equal(a.y_mix[:BATCH + 3], b.y_mix[:BATCH + 3])


def _roundtrip(w):
    buf = io.BytesIO()
    torch.save(w, buf)
    size = buf.tell()
    buf.seek(0)
    return torch.load(buf, weights_only=False), size


@pytest.mark.parametrize("kind", ["partial", "gem"])
def test_pickle_round_trip_gives_the_same_next_step(kind):
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.exemplar import batch_source
    tasks = _tasks()
    w = _wrapper(kind, True)
    _run(w, [byte for byte, _ in tasks], steps=2)
    state = w.__getstate__()
    rows = state["memory_x"] if kind == "gem" else state["_rows_x"]
    assert rows.dtype == torch.uint8 and "lut" not in state
    assert all(not v.is_cuda and v.dtype == torch.float32 for v in state["frame_norm"])
    w2, _ = _roundtrip(w)
    assert w2.frame_norm is not None and all(torch.equal(u, v) for u, v in zip(w2.frame_norm, w.frame_norm))
    assert w2.lut.is_cuda and torch.equal(_bits(w2.lut), _bits(w.lut))
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
        loader = DeviceLoader(tasks[1][0], BATCH, True, DEV)
        x, y = next(iter(loader))
        out = v.observe(x, 1, y, batch_source(loader)) if kind == "gem" else v.observe_FT(x, 1, y, batch_source(loader))
        res.append((out[0].clone(), out[1].clone(), [p.detach().clone() for p in v.parameters()]))
    assert torch.equal(_bits(res[0][0].reshape(1)), _bits(res[1][0].reshape(1))) and torch.equal(res[0][1], res[1][1])
    for p, q in zip(res[0][2], res[1][2]):
        assert torch.equal(_bits(p), _bits(q))


def test_the_pickle_of_a_byte_store_is_smaller():
    """The store rows dominate the pickle of a wrapper with a small net: bytes against floats."""
    tasks = _tasks()
    sizes = []
    for byte in (True, False):
        w = _wrapper("partial", byte)
        _run(w, [d[0 if byte else 1] for d in tasks], steps=1)
        sizes.append(_roundtrip(w)[1])
    rows = 2 * N_MEM * 3 * (HW + MARGIN) ** 2
    assert sizes[1] - sizes[0] >= 3 * rows - 4096                  # 4 bytes an element against 1, the rest is the same


def test_a_wrapper_refuses_the_other_kind_of_frames_on_the_device():
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.exemplar import batch_source
    tasks = _tasks()
    for kind in ("partial", "gem"):
        for byte in (True, False):
            w = _wrapper(kind, byte)
            loader = DeviceLoader(tasks[0][1 if byte else 0], BATCH, True, DEV)     # the other kind
            x, y = next(iter(loader))
            with pytest.raises(ValueError, match="store"):
                w.observe_FT(x, 0, y, batch_source(loader))
            if kind == "gem":
                with pytest.raises(ValueError, match="store"):
                    w.fill_buffer(0, x, y, batch_source(loader))


# ---------------------------------------------------------------------------------------------- gem_main.main
def _seeds(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _byte_dicts(root):
    """The augmented byte files of two synthetic tasks (frames 3 x 36 x 36, crops 32 x 32), loaded to the device."""
    from clsurvey_amd.data import load_task_datasets
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(80, 20, 20), hw=32, noise=0.4,
                               name="u8", u8_frames=True, rnd_margin=4)
    return [load_task_datasets(ds.get_task_dataset_path(str(t), rnd_transform=True), DEV) for t in (1, 2)]


def _base_model(path):
    from clsurvey_amd import models
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4), path)
    return path


def test_rehearsal_partial_mem_entry_builds_then_loads_a_byte_store(tmp_path):
    from clsurvey_amd.data import ByteTaskDataset
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dicts = _byte_dicts(root)
    assert all(isinstance(d["train"], ByteTaskDataset) and d["train"].transform is not None for d in dicts)
    prev = _base_model(os.path.join(root, "prev.pth.tar"))
    common = dict(n_outputs=8, method="baseline_rehearsal_partial_mem", n_memories=6, n_tasks=2, postprocess=False, n_epochs=1,
                  batch_size=16, lr=1e-2, exemplar_dtype="uint8")
    _seeds(11)
    m1, acc1 = gem_main.main(dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0],
                                  is_scratch_model=True, save_path=os.path.join(root, "t1")), [4, 4], device=DEV)
    assert m1.store_x.dtype == torch.uint8 and tuple(m1.store_x.shape) == (12, 3, 36, 36) and m1.filled == [6, 0]
    assert int(m1.store_x[:6].sum(dim=(1, 2, 3)).min()) > 0 and int(m1.store_x[6:].sum()) == 0 and 0.0 <= acc1 <= 1.0
    assert torch.equal(m1.frame_norm[0], dicts[0]["train"].mean) and torch.equal(m1.frame_norm[1], dicts[0]["train"].std)
    saved = os.path.join(root, "t1", "best_model.pth.tar")
    m2, acc2 = gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=saved, dataset_path=dicts[1],
                                  is_scratch_model=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert m2.store_x.dtype == torch.uint8 and m2.filled == [6, 6] and m2.last_path == "fused" and len(m2.last_gather) > 0
    assert int(m2.store_x[6:].sum(dim=(1, 2, 3)).min()) > 0 and 0.0 <= acc2 <= 1.0
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())
    # the loaded wrapper's store kind has to match the argument
    with pytest.raises(ValueError, match="exemplar store is uint8"):
        gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=saved, is_scratch_model=False, exemplar_dtype="float32",
                           dataset_path={s: d.decoded() for s, d in dicts[1].items()}, save_path=os.path.join(root, "t2f")), [4, 4],
                      device=DEV)


def test_gem_entry_builds_then_loads_a_byte_store(tmp_path):
    from clsurvey_amd.methods import gem_main
    root = str(tmp_path)
    dicts = _byte_dicts(root)
    prev = _base_model(os.path.join(root, "SI", "prev.pth.tar"))
    common = dict(n_outputs=8, method="gem", n_memories=6, n_tasks=2, n_epochs=1, batch_size=16, lr=1e-2, memory_strength=0.5,
                  exemplar_dtype="uint8")
    _seeds(12)
    wrapped = os.path.join(root, "t1", "best_model.pth.tar")
    gem_main.main(dict(common, task_name="1", task_count=1, prev_model_path=prev, dataset_path=dicts[0], is_scratch_model=True,
                       postprocess=True, save_path=wrapped), [4, 4], device=DEV)
    w = torch.load(wrapped, weights_only=False)
    assert w.memory_x.dtype == torch.uint8 and tuple(w.memory_x.shape) == (2, 6, 3, 36, 36) and w.frame_norm is not None
    assert int(w.memory_x[0].sum(dim=(1, 2, 3)).min()) > 0 and int(w.memory_x[1].sum()) == 0
    m2, acc2 = gem_main.main(dict(common, task_name="2", task_count=2, prev_model_path=wrapped, dataset_path=dicts[1],
                                  is_scratch_model=False, postprocess=False, save_path=os.path.join(root, "t2")), [4, 4], device=DEV)
    assert m2.memory_x.dtype == torch.uint8 and m2.observed_tasks == [0, 1] and 0.0 <= acc2 <= 1.0
    assert int(m2.memory_x[1].sum(dim=(1, 2, 3)).min()) > 0 and torch.equal(m2.memory_x[0], w.memory_x[0])
    assert all(bool(torch.isfinite(p).all()) for p in m2.parameters())


# ---------------------------------------------------------------------------------------------- through the driver
def test_rehearsal_partial_mem_through_the_driver_with_byte_exemplars(tmp_path):
    from clsurvey_amd import models
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
            "--results_root", root, "--synthetic", "2,4,160,40,40,32", "--u8_frames", "--rnd_margin", "4", "--u8_exemplars",
            "--method_name", "finetuning_rehearsal_partial_mem", "--test", "--mem_per_task", "24"]
    out = driver.main(argv)
    res = out["results"]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    assert sorted(res) == [0, 1] and len(accs) > 0 and all(a == a and 0.0 <= a <= 100.0 for a in accs)
    for k, path in enumerate(out["model_paths"], start=1):
        w = torch.load(path, weights_only=False)
        assert w.store_x.dtype == torch.uint8 and tuple(w.store_x.shape) == (48, 3, 36, 36) and w.filled[:k] == [24] * k
        assert w.frame_norm is not None and int(w.store_x[:24 * k].sum(dim=(1, 2, 3)).min()) > 0
    with pytest.raises(SystemExit, match="--u8_exemplars belongs with"):
        driver.main([a for a in argv if a != "--u8_frames"])
