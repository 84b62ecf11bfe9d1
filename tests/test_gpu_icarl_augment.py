"""iCaRL on augmented tasks, on the GPU.  The step-assembly entries clhip_icarl_assemble_* against a CPU slicing restatement and
against the composition of the entries they replace (copies and one shared device body: bitwise, no tolerance), their safety
rule; IcarlNet in frame mode without freedom against its crop-mode run, with a margin against a restatement of its own draws
(herding view, replay draws, class-mean view), a byte store against the fp32 run on the decoded split, the pickle, the mode
checks; ICARL through the driver on augmented tasks."""
import copy
import functools
import io
import os
import random
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, STORE_ROWS = 5, 12                                             # (the store tensors carry one spare row behind store_rows)
GATHER = [9, 0, 3, 11, 9, 1, 8]                                   # E = 7, store row 9 twice
GUARD = 4                                                         # guard floats before and after an output (keeps 16-byte alignment)
FILL = -7.0


def restate(frames, rows, params, th, tw):
    """torchvision's crop, then hflip, of frames[rows[e]] with params[e] = (top, left, flip), on the CPU."""
    out = [frames[g, :, top:top + th, left:left + tw] for g, (top, left, _) in zip(rows, params.tolist())]
    return torch.stack([v.flip(-1) if flip else v for v, (_, _, flip) in zip(out, params.tolist())])


def decode(frames, lut):
    """What byte frames mean: lut[c][v] (indexing, no arithmetic)."""
    if frames.dtype != torch.uint8:
        return frames
    return torch.stack([lut[c][frames[:, c].long()] for c in range(frames.shape[1])], 1)


def _crop_params(Hs, Ws, th, tw):
    """Offsets 0 and the maximum on both axes, both flip values, two rows for store row 9."""
    mt, ml = Hs - th, Ws - tw
    return torch.tensor([[0, 0, 0], [mt, ml, 1], [0, ml, 1], [mt, 0, 0], [mt // 2, min(1, ml), 1], [min(1, mt), ml // 2, 0],
                         [mt, min(3, ml), 1]], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _case(geo, n_out, byte, resized):
    """Made once per (geometry, target width, store kind, transform) and never written to (launches work on device copies)."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip, norm_lut
    C, Hs, Ws, th, tw = geo
    gen = torch.Generator().manual_seed(sum(geo) + 100 * n_out + int(byte))
    if resized:                                                   # the spec's draws, the full frame and a 1 x 1 window
        drawn = draw_resized_crop_flip(len(GATHER) - 2, RandomResizedCropFlip((th, tw)), (Hs, Ws), gen)
        params = torch.cat([drawn, torch.tensor([[0, 0, Hs, Ws, 1], [Hs - 1, Ws - 1, 1, 1, 0]], dtype=torch.int32)]).contiguous()
    else:
        params = _crop_params(Hs, Ws, th, tw)
    if byte:
        store = torch.randint(0, 256, (STORE_ROWS + 1, C, Hs, Ws), generator=gen, dtype=torch.uint8)
        lut = norm_lut(torch.rand(C, generator=gen), 0.2 + torch.rand(C, generator=gen))
    else:
        store, lut = torch.randn((STORE_ROWS + 1, C, Hs, Ws), generator=gen), None
    return dict(geo=geo, n_out=n_out, resized=resized, lut=lut, store=store,
                x=torch.randn((B, C, th, tw), generator=gen), y=torch.randint(1, 20, (B,), generator=gen),
                store_t=torch.randn((STORE_ROWS + 1, n_out), generator=gen),
                gather=torch.tensor(GATHER, dtype=torch.int32), params=params)


def _entry(c):
    from clsurvey_amd import ops
    name = "icarl_assemble_%scrop_flip%s" % ("resized_" if c["resized"] else "", "_u8" if c["lut"] is not None else "")
    return getattr(ops, name)


def _guarded(n, offset=0):
    """A device buffer of n floats with GUARD floats (and `offset` more in front) around it, all FILL; (whole, view)."""
    buf = torch.full((GUARD + offset + n + GUARD,), FILL, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + n]
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def _launch(c, b=B, e=len(GATHER), off_x=0, off_t=0, null_x=False):
    """Runs case c's entry on device copies.  Returns CPU (x_mix [b + e, C, th, tw], y_mix, t_mix [b + e, n_out]) after checking
    that the guard floats around x_mix and t_mix are untouched."""
    C, Hs, Ws, th, tw = c["geo"]
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    row = C * th * tw
    xbuf, xm = _guarded((b + e) * row, off_x)
    tbuf, tm = _guarded((b + e) * c["n_out"], off_t)
    ym = torch.full((b + e,), 99, dtype=torch.int64, device=DEV)
    table = () if c["lut"] is None else (d["lut"],)
    _entry(c)(c["geo"], *table, None if null_x else d["x"][:b].contiguous(), None if null_x else d["y"], b,
              d["store"][:STORE_ROWS], d["gather"][:e] if e else None, d["params"][:e].contiguous() if e else None,
              d["store_t"], xm, ym, tm.view(b + e, c["n_out"]))
    torch.cuda.synchronize()
    for buf, n, off in ((xbuf, (b + e) * row, off_x), (tbuf, (b + e) * c["n_out"], off_t)):
        host = buf.cpu()
        assert bool((host[:GUARD + off] == FILL).all()) and bool((host[GUARD + off + n:] == FILL).all())
    return xm.cpu().view(b + e, C, th, tw), ym.cpu(), tm.cpu().view(b + e, c["n_out"])


def _windows_on_device(c, rows, params):
    """The loaders' gather over a one-task table laid over the store: crops [n, C, th, tw] (CPU)."""
    from clsurvey_amd import ops
    store = c["store"].to(DEV)
    table = ops.task_table([store], [torch.zeros(store.shape[0], dtype=torch.int64, device=DEV)], [store.shape[0]], [0], DEV)
    idx, params = rows.to(DEV).long(), params.to(DEV).contiguous()
    kind = "resized_crop_flip" if c["resized"] else "crop_flip"
    if c["lut"] is not None:
        return getattr(ops, "gather_tasks_%s_u8" % kind)(table, c["geo"], c["lut"].to(DEV), idx, params)[0].cpu()
    return getattr(ops, "gather_tasks_%s" % kind)(table, c["geo"], idx, params)[0].cpu()


def _expect(c, b=B, e=len(GATHER)):
    """(x_mix, y_mix, t_mix) of a launch over case c: the copy rows, the windows (crop: CPU slicing of the decoded store; resized:
    the loaders' resizing gather, the kernel's yardstick), zeros for the exemplar labels, the stored target rows behind b rows of
    prefill."""
    C, Hs, Ws, th, tw = c["geo"]
    rows = c["gather"][:e].long()
    if e == 0:
        ex = torch.zeros((0, C, th, tw))
    elif c["resized"]:
        ex = _windows_on_device(c, rows, c["params"][:e])
    else:
        ex = restate(decode(c["store"], c["lut"]), rows.tolist(), c["params"][:e], th, tw)
    return (torch.cat([c["x"][:b], ex]), torch.cat([c["y"][:b], torch.zeros(e, dtype=torch.int64)]),
            torch.cat([torch.full((b, c["n_out"]), FILL), c["store_t"].index_select(0, rows)]))


def _composition(c, b=B, e=len(GATHER)):
    """What the entry replaces: the parent's frame-mode assembly with no ring rows (labels 0 in the store), then
    clhip_rehearsal_assemble over the target rows."""
    from clsurvey_amd import _lib, ops
    C, Hs, Ws, th, tw = c["geo"]
    d = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    xm = torch.full((b + e, C, th, tw), FILL, device=DEV)
    ym = torch.full((b + e,), 99, dtype=torch.int64, device=DEV)
    tm = torch.full((b + e, c["n_out"]), FILL, device=DEV)
    lab = torch.zeros(STORE_ROWS + 1, dtype=torch.int64, device=DEV)
    scratch = torch.empty(e, dtype=torch.int64, device=DEV)
    name = "rehearsal_assemble_%scrop_flip%s" % ("resized_" if c["resized"] else "", "_u8" if c["lut"] is not None else "")
    table = () if c["lut"] is None else (d["lut"],)
    getattr(ops, name)(c["geo"], *table, d["x"][:b].contiguous(), d["y"], b, None, None, d["store"][:STORE_ROWS], lab, 0, 0,
                       d["gather"][:e], d["params"][:e].contiguous(), xm, ym)
    _lib.check(_lib.lib().clhip_rehearsal_assemble(None, None, 0, c["n_out"], d["store_t"].data_ptr(), lab.data_ptr(), STORE_ROWS, 0, 0,
                                                   d["gather"].data_ptr(), e, tm[b:].data_ptr(), scratch.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "clhip_rehearsal_assemble")
    torch.cuda.synchronize()
    return xm.cpu(), ym.cpu(), tm.cpu()


def _same(got, want):
    return all(torch.equal(g.view(-1).view(torch.uint8), w.view(-1).view(torch.uint8)) for g, w in zip(got, want))


CROP_GEOMETRIES = [(1, 9, 11, 5, 6), (3, 10, 12, 8, 8), (3, 8, 8, 8, 8), (3, 20, 20, 16, 16)]
RESIZED_GEOMETRIES = [(3, 20, 20, 16, 16), (1, 9, 11, 5, 6), (2, 6, 13, 8, 8)]           # the last one: every window enlarged (h < th)


def _ids(geos):
    return ["%dx%dx%d_to_%dx%d" % g for g in geos]


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("n_out", [12, 5], ids=["targets_vec", "targets_scalar"])
@pytest.mark.parametrize("geo", CROP_GEOMETRIES, ids=_ids(CROP_GEOMETRIES))
def test_crop_flip_kernel_is_bitwise_the_restatement_and_the_composition(geo, n_out, byte):
    """The scalar path at odd sizes / vector stores from unaligned source lines / no freedom / a 16 x 16 crop; target rows of 12
    floats (16-byte accesses) and of 5 (scalar).  x_mix, labels_mix and t_mix against the CPU restatement and against the two
    launches the entry replaces; the guard floats around the outputs stay (checked in _launch)."""
    c = _case(geo, n_out, byte, False)
    got = _launch(c)
    assert _same(got, _expect(c)) and _same(got, _composition(c))
    assert got[1][B:].tolist() == [0] * len(GATHER)
    if geo[1] > geo[3] and geo[2] > geo[4]:
        assert not torch.equal(got[0][B], got[0][B + 4])           # store row 9 under two parameter rows
    assert torch.equal(got[2][B], got[2][B + 4])                   # ... and its one target row twice


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("geo", RESIZED_GEOMETRIES, ids=_ids(RESIZED_GEOMETRIES))
def test_resized_kernel_is_bitwise_the_resizing_gather(geo, byte):
    """Windows of draw_resized_crop_flip, the full frame and a 1 x 1 window: the exemplar rows are bitwise what
    gather_tasks_resized_crop_flip[_u8] gives for the same frames and windows, the target rows bitwise the stored ones; and the
    whole is the composition of the parent's entries."""
    c = _case(geo, 12, byte, True)
    got = _launch(c)
    assert _same(got, _expect(c)) and _same(got, _composition(c))
    assert bool(torch.isfinite(got[0]).all()) and float(got[0][B:].abs().sum()) > 0


@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized"])
def test_kernel_without_current_rows_and_without_exemplars(resized):
    """B = 0 with x = labels = NULL (the class-mean view's form); E = 0 with nothing of the store."""
    c = _case((3, 10, 12, 8, 8), 12, False, resized)
    assert _same(_launch(c, b=0, null_x=True), _expect(c, b=0))
    assert _same(_launch(c, b=0), _expect(c, b=0))
    assert _same(_launch(c, e=0), _expect(c, e=0))
    cb = _case((3, 10, 12, 8, 8), 12, True, resized)
    assert _same(_launch(cb, b=0, null_x=True), _expect(cb, b=0))


@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized"])
def test_unaligned_outputs_take_the_plain_path(resized):
    """tw % 4 == 0 and n_outputs % 4 == 0, but x_mix / t_mix 4 bytes off a 16-byte boundary: no 16-byte accesses, the same
    bytes, the floats around them untouched."""
    c = _case((3, 10, 12, 8, 8), 12, False, resized)
    want = _expect(c)
    assert _same(_launch(c, off_x=1), want) and _same(_launch(c, off_t=1), want) and _same(_launch(c, off_x=1, off_t=1), want)


@pytest.mark.parametrize("bad", ["gather_row", "top", "flip", "h"])
@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_bad_rows_copy_nothing_and_get_label_minus_one(bad, byte):
    """A gather row equal to store_rows, top one past its range, flip = 2, and for a resized window h = 0: that row keeps its
    prefill in x_mix AND in t_mix and gets label -1; every other row is exact.  (The store tensors carry a spare row and the bad
    row is in the middle of the store: a kernel without the rule would read inside this test's allocations and fail by value.)"""
    resized = bad == "h"
    geo = (3, 10, 12, 8, 8)
    ok = _case(geo, 12, byte, resized)
    for n_out in (12, 5):
        ok = _case(geo, n_out, byte, resized)
        c = copy.deepcopy(ok)
        if bad == "gather_row":
            c["gather"][2] = STORE_ROWS
        elif bad == "top":
            c["params"][2, 0] = geo[1] - geo[3] + 1
        elif bad == "flip":
            c["params"][2, 2] = 2
        else:
            c["params"][2, 2] = 0
        xm, ym, tm = _launch(c)
        w_xm, w_ym, w_tm = (v.clone() for v in _expect(ok))
        w_xm[B + 2], w_ym[B + 2], w_tm[B + 2] = FILL, -1, FILL
        assert _same((xm, ym, tm), (w_xm, w_ym, w_tm))


# ---------------------------------------------------------------------------------------------- the wrapper
HW, NCLS, N_TRAIN, BATCH, N_MEM, N_APPEND, HERD_BATCH, EVAL_BATCH = 16, 4, 24, 8, 8, 3, 5, 3
MEAN, STD = torch.tensor([0.45, 0.5, 0.55]), torch.tensor([0.25, 0.2, 0.3])


def _net():
    from clsurvey_amd.models import VGGSlim
    return VGGSlim(cfg=[8, "M", 16, "M"], num_classes=NCLS, classifier_inputdim=16 * 4 * 4, classifier_dim1=32, classifier_dim2=32,
                   dropout=True, batch_norm=False)


def _spec(kind, p):
    from clsurvey_amd.data import RandomCropFlip, RandomResizedCropFlip
    return RandomResizedCropFlip((HW, HW), p=p) if kind == "resized" else RandomCropFlip((HW, HW), p)


@functools.lru_cache(maxsize=None)
def _tasks(margin, p, kind="crop", byte=False, seed=21):
    """Two tasks of 24 frames 3 x (16 + margin)^2 on the device, never written to: [(plain centre crops, augmented frames)]; byte:
    [(the decoded augmented split, the augmented byte split)]."""
    from clsurvey_amd.data import ByteTaskDataset, TensorTaskDataset
    gen = torch.Generator().manual_seed(seed)
    out = []
    names = [str(k) for k in range(NCLS)]
    for _ in range(2):
        y = torch.arange(N_TRAIN)[torch.randperm(N_TRAIN, generator=gen)] % NCLS         # 6 images per class
        x = torch.randn((N_TRAIN, 3, HW + margin, HW + margin), generator=gen) + (y[:, None, None, None] - 1.5) * 0.5
        if byte:
            xb = (x * 40 + 128).clamp(0, 255).to(torch.uint8)
            aug = ByteTaskDataset(xb.to(DEV), y.to(DEV), names, MEAN, STD, transform=_spec(kind, p))
            out.append((aug.decoded(), aug))
        else:
            lo = margin // 2
            out.append((TensorTaskDataset(x[:, :, lo:lo + HW, lo:lo + HW].to(DEV), y.to(DEV), names),
                        TensorTaskDataset(x.to(DEV), y.to(DEV), names, transform=_spec(kind, p))))
    return out


def _wrapper(spec, frame_shape, segmented=False, frame_norm=None):
    from clsurvey_amd.methods.icarl import IcarlNet
    torch.manual_seed(5)
    kw = dict(exemplar_transform=spec, frame_shape=frame_shape, frame_norm=frame_norm) if spec is not None else {}
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
    """Two tasks from a fixed RNG state: `steps` observe steps each, then manage_memory.  Returns the losses."""
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.exemplar import batch_source
    _seed(9)
    losses = []
    for t, dset in enumerate(dsets):
        _setup(w, t)
        loader = DeviceLoader(dset, BATCH, True, DEV)
        for k, (x, y) in enumerate(loader):
            if k == steps:
                break
            src = {"source": batch_source(loader)} if w.exemplar_transform is not None else {}
            before = (torch.get_rng_state(), np.random.get_state(), random.getstate())
            out = w.observe(x, t, y, **src)
            losses.append(out[0].clone())
            if after_step is not None:
                after_step(w, t, x, y, before)
        w.manage_memory(t, _herd_args(dset))
        if after_herding is not None:
            after_herding(w, t, dset)
    torch.cuda.synchronize()
    return torch.cat([v.reshape(1) for v in losses]).cpu()


@functools.lru_cache(maxsize=None)
def _probe():
    return torch.randn((7, 3, HW, HW), generator=torch.Generator().manual_seed(77)).to(DEV)


def _codes(w):
    args = types.SimpleNamespace(batch_size=EVAL_BATCH)
    return torch.stack([w(_probe(), t, args=args).cpu() for t in range(2)])


@pytest.mark.parametrize("segmented", [False, True], ids=["fused", "segmented"])
def test_frame_mode_without_freedom_is_the_crop_mode_run(segmented):
    """Frames of the crop size and p = 0: the herding view is the frames themselves, every replay window is the whole frame.
    Rankings, store_t, losses, parameters and NME codes are bitwise those of the crop-mode wrapper from the same RNG state, and
    the frame store equals the crop store."""
    tasks = _tasks(0, 0.0)
    a = _wrapper(None, None, segmented)
    rank_a, rank_b = [], []
    la = _run(a, [plain for plain, _ in tasks], after_herding=lambda w, t, d: rank_a.append(w.last_ranking[0].cpu().tolist()))
    b = _wrapper(_spec("crop", 0.0), (3, HW, HW), segmented)
    lb = _run(b, [aug for _, aug in tasks], after_herding=lambda w, t, d: rank_b.append(w.last_ranking[0].cpu().tolist()))
    assert a.exemplar_transform is None and b.exemplar_transform is not None
    assert a.last_path == b.last_path == ("segmented" if segmented else "fused")
    assert rank_a == rank_b and len(rank_a) == 2 and len(rank_a[1]) >= 2 * NCLS
    assert b.last_gather == a.last_gather and len(b.last_gather) == N_APPEND and int(b.last_exemplar_params.abs().sum()) == 0
    assert int(b.last_herd_params.abs().sum()) == 0 and a.last_exemplar_params is None
    assert torch.equal(la, lb) and len(la) == 6 and bool(torch.isfinite(la).all()) and float((la[0] - la[-1]).abs()) > 0
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert a.class_len == b.class_len == [2] * 8 and a.exemplar_count == b.exemplar_count == 2
    assert torch.equal(a.store_t, b.store_t) and float(a.store_t.abs().sum()) > 0
    assert torch.equal(a.store_x, b.store_x) and float(a.store_x.abs().sum()) > 0
    assert b.store_ext.tolist() == [[HW, HW]] * (2 * N_MEM)
    ca, cb = _codes(a), _codes(b)
    assert torch.equal(ca, cb) and float(ca.sum()) == 2 * 7


def _view_crops(w, frames, rows, params):
    """Crops of frames[rows] under params: a plain crop is restated on the CPU (slicing of the decoded frames); a resized window
    goes through the loaders' resizing gather, which has its own tests against the filter's restatement."""
    from clsurvey_amd import ops
    from clsurvey_amd.data import RandomResizedCropFlip
    rows = [int(r) for r in rows]
    if not isinstance(w.exemplar_transform, RandomResizedCropFlip):
        dec = decode(frames.cpu(), None if w.frame_norm is None else w.lut.cpu())
        return restate(dec, rows, params, HW, HW).to(DEV)
    table = ops.task_table([frames], [torch.zeros(frames.shape[0], dtype=torch.int64, device=DEV)], [frames.shape[0]], [0], DEV)
    idx = torch.tensor(rows, dtype=torch.int64, device=DEV)
    if w.frame_norm is not None:
        return ops.gather_tasks_resized_crop_flip_u8(table, w.geometry, w.lut, idx, params.to(DEV).contiguous())[0]
    return ops.gather_tasks_resized_crop_flip(table, w.geometry, idx, params.to(DEV).contiguous())[0]


@pytest.mark.parametrize("kind", ["crop", "resized"])
def test_with_a_margin_herding_and_replay_follow_their_own_draws(kind):
    """Frames 3 x 20 x 20 -> 16 x 16, p = 0.5.  After manage_memory: last_ranking is w.herd over w.features of the restated
    herding-view crops (chunks of the engine's batch), the store rows are the winners' frames with their extents, store_t is
    forward_training of the winners' restated crops.  After every observe: x_mix[B:N) is the restatement of
    store_x[last_gather] under last_exemplar_params, t_mix[B:N) is store_t[last_gather], consecutive steps draw different
    tables, and the global generators stand where the crop-mode step's host draws (plan) leave them."""
    from clsurvey_amd.methods.icarl import VIEW_HERD, VIEW_MEANS, compute_offsets, mean_weights
    tasks = _tasks(4, 0.5, kind)
    w = _wrapper(_spec(kind, 0.5), (3, HW + 4, HW + 4))
    assert tuple(w.store_x.shape) == (2 * N_MEM, 3, 20, 20) and w.in_shape == (3, HW, HW) and w.params_width == (5 if kind == "resized" else 3)
    seen = []

    def after_step(w, t, x, y, before):
        n, E = x.shape[0], len(w.last_gather)
        assert E == (N_APPEND if t else 0) and tuple(w.last_exemplar_params.shape) == (E, w.params_width)
        assert torch.equal(w.x_mix[:n], x) and torch.equal(w.y_mix[:n], y)
        after = (torch.get_rng_state(), np.random.get_state(), random.getstate())
        torch.set_rng_state(before[0])
        np.random.set_state(before[1])
        random.setstate(before[2])
        w.plan(t)                                                  # the host draws of a crop-mode step
        assert torch.equal(torch.get_rng_state(), after[0]) and random.getstate() == after[2]
        assert np.array_equal(np.random.get_state()[1], after[1][1]) and np.random.get_state()[2] == after[1][2]
        if E:
            want = _view_crops(w, w.store_x, w.last_gather, w.last_exemplar_params)
            assert torch.equal(w.x_mix[n:n + E], want) and int(w.y_mix[n:n + E].abs().sum()) == 0
            assert torch.equal(w.t_mix[n:n + E], w.store_t[torch.tensor(w.last_gather, device=DEV)])
            seen.append(w.last_exemplar_params.clone())

    def after_herding(w, t, dset):
        n, count = len(dset), w.exemplar_count
        assert count == 2 * N_MEM // (NCLS * (t + 1))
        params = w.last_herd_params
        assert torch.equal(params, w.view_params(t, VIEW_HERD, w._full_ext(n))) and tuple(params.shape) == (n, w.params_width)
        w.net.train(False)
        w._dropout(1)
        crops = _view_crops(w, dset.x, range(n), params)
        feats = w.features(crops)
        order = torch.sort(dset.y, stable=True)[1]
        sizes = torch.bincount(dset.y, minlength=NCLS).cpu().tolist()
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        ks = [min(count, m) for m in sizes]
        wts = torch.from_numpy(np.concatenate([mean_weights(m, HERD_BATCH) for m in sizes])).to(DEV)
        ranking, offs = w.herd(feats.index_select(0, order), [(int(bounds[c]), int(bounds[c + 1])) for c in range(NCLS)], wts, ks)
        assert torch.equal(ranking, w.last_ranking[0]) and list(offs) == list(w.last_ranking[1])
        o1, _ = compute_offsets(t, w.cum_nc_per_task)
        wins, targets = [], []
        for c in range(NCLS):
            r0, m = w._block(o1 + c)
            assert m == ks[c] == count
            win = order[int(bounds[c]) + ranking[int(offs[c]):int(offs[c + 1])].long()]
            assert torch.equal(w.store_x[r0:r0 + m], dset.x[win])
            assert w.store_ext[r0:r0 + m].tolist() == [[HW + 4, HW + 4]] * m
            wins.append(win)
            targets.append(w.store_t[r0:r0 + m])
        # (all winners in one call, class after class: the chunks of the engine's batch manage_memory itself ran)
        assert torch.equal(torch.cat(targets), w.forward_training(crops[torch.cat(wins)], t))
        assert float(torch.cat(targets).abs().sum()) > 0

    losses = _run(w, [aug for _, aug in tasks], after_step=after_step, after_herding=after_herding)
    assert len(seen) == 3 and bool(torch.isfinite(losses).all()) and w.last_path == "fused"
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    if kind == "crop":
        assert 0 < int(torch.cat(seen)[:, :2].max()) <= 4 and 0 < int(w.last_herd_params[:, :2].max()) <= 4
    # class_means: the means of w.features of the restated class-mean-view crops
    for t in range(2):
        o1, o2 = compute_offsets(t, w.cum_nc_per_task)
        rows = [c * w.exemplar_count + e for c in range(o1, o2) for e in range(w.class_len[c])]
        params = w.view_params(t, VIEW_MEANS, w.store_ext[torch.tensor(rows)])
        assert not torch.equal(params, w.last_herd_params[:len(rows)])
        w._eval_dropout(1)
        feats = w.features(_view_crops(w, w.store_x, rows, params))
        want, lo = [], 0
        for c in range(o1, o2):
            m = w.class_len[c]
            wt = torch.from_numpy(mean_weights(m, EVAL_BATCH)).to(DEV).double()
            want.append((feats[lo:lo + m].double() * wt[:, None]).sum(0).float())
            lo += m
        w._means = {}
        got = w.class_means(t, EVAL_BATCH)
        assert torch.equal(got, torch.stack(want)) and got is w.class_means(t, EVAL_BATCH)
    codes = _codes(w)
    w._means = {}
    assert torch.equal(codes, _codes(w)) and float(codes.sum()) == 2 * 7                    # an evaluation is reproducible


@pytest.mark.parametrize("kind", ["crop", "resized"])
def test_byte_store_is_bitwise_the_fp32_run_on_the_decoded_split(kind):
    tasks = _tasks(4, 0.5, kind, True)
    a = _wrapper(_spec(kind, 0.5), (3, HW + 4, HW + 4))
    la = _run(a, [dec for dec, _ in tasks])
    b = _wrapper(_spec(kind, 0.5), (3, HW + 4, HW + 4), frame_norm=(MEAN, STD))
    lb = _run(b, [aug for _, aug in tasks])
    assert a.store_dtype == torch.float32 and b.store_dtype == torch.uint8 and b.store_x.dtype == torch.uint8
    assert torch.equal(la, lb) and bool(torch.isfinite(la).all()) and b.last_gather == a.last_gather
    assert torch.equal(a.last_exemplar_params, b.last_exemplar_params) and torch.equal(a.last_herd_params, b.last_herd_params)
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert a.class_len == b.class_len and torch.equal(a.store_t, b.store_t)
    assert torch.equal(a.store_x.cpu(), decode(b.store_x.cpu(), b.lut.cpu())) and float(a.store_x.abs().sum()) > 0
    assert torch.equal(_codes(a), _codes(b))


def _roundtrip(w):
    buf = io.BytesIO()
    torch.save(w, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
def test_pickle_round_trip_gives_the_same_next_step_and_codes(byte):
    from clsurvey_amd.data import DeviceLoader
    from clsurvey_amd.methods.exemplar import batch_source
    tasks = _tasks(4, 0.5, "crop", byte)
    w = _wrapper(_spec("crop", 0.5), (3, HW + 4, HW + 4), frame_norm=(MEAN, STD) if byte else None)
    _run(w, [aug for _, aug in tasks], steps=1)
    w.view_seed = 3
    w.store_ext[:2, 0] = 18                                        # (extents other than the full frame travel too)
    state = w.__getstate__()
    n = sum(w.class_len)
    assert state["_rows_x"].dtype == w.store_dtype and tuple(state["_rows_x"].shape) == (n, 3, 20, 20) and n == 16
    assert tuple(state["_rows_ext"].shape) == (n, 2) and not state["_rows_ext"].is_cuda and tuple(state["_rows_t"].shape) == (n, 2 * NCLS)
    assert not {"store_x", "store_t", "store_ext", "last_gather", "last_exemplar_params", "last_herd_params", "lut"} & set(state)
    w2 = _roundtrip(w)
    assert w2.exemplar_transform.size == (HW, HW) and w2.frame_shape == (3, 20, 20) and w2.view_seed == 3
    assert (w2.frame_norm is not None) == byte and w2.store_dtype == w.store_dtype and w2.last_gather is None
    assert torch.equal(w2.store_x, w.store_x) and torch.equal(w2.store_t, w.store_t) and torch.equal(w2.store_ext, w.store_ext)
    codes = [_codes(v) for v in (w, w2)]
    assert torch.equal(codes[0], codes[1])
    res = []
    for v in (w, w2):
        _setup(v, 1)                                               # what main() does after torch.load
        _seed(15)
        loader = DeviceLoader(tasks[1][1], BATCH, True, DEV)
        x, y = next(iter(loader))
        loss, hits, _ = v.observe(x, 1, y, batch_source(loader))
        E = len(v.last_gather)                                     # (8 classes share the 3 exemplars of a step; task 0's are replayed)
        res.append((loss.clone(), hits.clone(), v.x_mix[:BATCH + E].clone(), v.last_exemplar_params,
                    [p.detach().clone() for p in v.parameters()]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert torch.equal(res[0][3], res[1][3]) and res[0][3].shape[0] >= 1 and res[0][3].shape[1] == 3
    for p, q in zip(res[0][4], res[1][4]):
        assert torch.equal(p, q)


def test_mode_checks():
    """A frame-mode wrapper refuses a plain batch and the reverse; manage_memory in frame mode refuses a split without a
    transform, a split of the other store kind and a byte split whose mean / std differ from the store's."""
    from clsurvey_amd.data import ByteTaskDataset
    from clsurvey_amd.methods.exemplar import BatchSource
    x = torch.randn(BATCH, 3, HW, HW, device=DEV)
    y = torch.randint(0, NCLS, (BATCH,), device=DEV)
    src = BatchSource(torch.randn(BATCH, 3, HW, HW, device=DEV), torch.arange(BATCH, device=DEV), torch.arange(BATCH), None)
    framed = _wrapper(_spec("crop", 0.0), (3, HW, HW))
    plain = _wrapper(None, None)
    for w, source in ((framed, None), (plain, src)):
        _setup(w, 0)
        with pytest.raises(ValueError):
            w.observe(x, 0, y, source)
        with pytest.raises(ValueError):
            w.observe_FT(x, 0, y, source)
    loss, hits = framed.observe_FT(x, 0, y, src)                   # (the source is only checked: nothing is copied from the batch)
    assert bool(torch.isfinite(loss).all())
    margin = _tasks(4, 0.5)
    w = _wrapper(_spec("crop", 0.5), (3, HW + 4, HW + 4))
    with pytest.raises(ValueError, match="carries no transform"):
        w.manage_memory(0, _herd_args(_tasks(0, 0.0)[0][0]))
    with pytest.raises(ValueError, match="the train split carries"):
        w.manage_memory(0, _herd_args(_tasks(4, 0.5, "resized")[0][1]))
    aug = _tasks(4, 0.5, "crop", True)[0][1]
    with pytest.raises(ValueError, match="byte store takes byte frames"):
        w.manage_memory(0, _herd_args(aug))                        # byte frames for an fp32 store
    wb = _wrapper(_spec("crop", 0.5), (3, HW + 4, HW + 4), frame_norm=(MEAN, STD))
    with pytest.raises(ValueError, match="byte store takes byte frames"):
        wb.manage_memory(0, _herd_args(margin[0][1]))              # float frames for a byte store
    other = ByteTaskDataset(aug.x, aug.y, aug.classes, MEAN + 0.125, STD, transform=aug.transform)
    with pytest.raises(ValueError, match="one table decodes a byte store"):
        wb.manage_memory(0, _herd_args(other))
    assert wb.class_len == [] and w.class_len == []
    wb.manage_memory(0, _herd_args(aug))
    assert wb.class_len == [4] * NCLS
    with pytest.raises(NotImplementedError, match="an augmented split"):          # crop mode: today's refusal, unchanged
        plain.manage_memory(0, _herd_args(margin[0][1]))


# ---------------------------------------------------------------------------------------------- through the driver
def _friendly_base_model(root):
    from clsurvey_amd import models
    torch.manual_seed(0)
    m = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(m, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))


def _common(root, *flags):
    return ["small_VGG9_cl_128_128", "--lr_grid", "1e-2,3e-3", "--num_epochs", "3", "--batch_size", "40", "--saving_freq", "100",
            "--results_root", root, "--synthetic", "2,4,160,40,40,32"] + list(flags)


def _icarl():
    from clsurvey_amd.methods import method as M
    icarl = M.parse("ICARL")
    icarl.static_hyperparams = {"mem_per_task": 16}
    return icarl


DRIVER_CASES = {"margin": (["--rnd_margin", "4", "--icarl_frames"], torch.float32, False),
                "resized": (["--rnd_resized", "4", "--icarl_frames", "--resized_exemplars"], torch.float32, True),
                "u8": (["--u8_frames", "--rnd_margin", "4", "--icarl_frames", "--u8_exemplars"], torch.uint8, False)}


@pytest.mark.parametrize("case", sorted(DRIVER_CASES))
def test_icarl_through_the_driver_on_augmented_tasks(tmp_path, case):
    """An SI first-task dump, then two tasks of ICARL --test on an augmented synthetic sequence: the run reaches the end, the
    accuracies (nearest mean of exemplars on the centre crops) are finite, the saved wrappers hold frames.
    Under RandomCrop (margin, u8) the task just learned is above chance (25 %).  test_icarl_through_driver's 35 % belongs to its
    own sequence (noise 0.4, 6 epochs); nothing says the reference clears it on this one, so the bound is chance.
    Under RandomResizedCrop only finiteness is asserted: this sequence's classes are pixel-aligned prototypes under noise 1.0, and
    a window of 8 - 100 % of the frame resized to 32 x 32 leaves no class signal in them.  The shared SI first-task training (no
    iCaRL code involved) ends at a training loss of ln 4 per sample, the uniform prediction; measured on task 1 after task 1 /
    after task 2: 10.0 % / 25.0 %, the same with 3, 8, 16 and 30 epochs, while the margin case goes from 32.5 % (3 epochs) to
    67.5 % (30).  No method can clear chance there, so a bound would test the data, not the method."""
    from clsurvey_amd.data import RandomResizedCropFlip
    from clsurvey_amd.framework import driver
    flags, dtype, resized = DRIVER_CASES[case]
    root = str(tmp_path)
    _friendly_base_model(root)
    driver.main(_common(root, *flags) + ["--method_name", "SI", "--runmode", "first_task_basemodel_dump"])
    out = driver.main(_common(root, *flags) + ["--method_name", "ICARL", "--test"], method=_icarl())
    res = out["results"]
    assert sorted(res) == [0, 1]
    accs = [a for i in res for a in res[i]["seq_res"][i]]
    print("accuracies", case, {i: res[i]["seq_res"][i] for i in res})
    assert len(accs) > 0 and all(np.isfinite(a) and 0.0 <= a <= 100.0 for a in accs)
    if not resized:
        assert all(res[i]["seq_res"][i][0] > 25.0 for i in res), res
    paths = out["model_paths"]
    assert len(paths) == 2
    for k, path in enumerate(paths, start=1):
        w = torch.load(path, weights_only=False)
        count = 32 // (4 * k)
        assert w.frame_shape == (3, 36, 36) and w.in_shape == (3, 32, 32) and w.exemplar_transform.size == (32, 32)
        assert isinstance(w.exemplar_transform, RandomResizedCropFlip) == resized
        assert w.store_dtype == dtype and w.store_x.dtype == dtype and tuple(w.store_x.shape) == (32, 3, 36, 36)
        assert w.exemplar_count == count and w.class_len == [count] * (4 * k) and w.observed_tasks == list(range(k))
        assert w.store_ext.tolist() == [[36, 36]] * 32
        assert float(w.store_x[:4 * k * count].float().abs().sum(dim=(1, 2, 3)).min()) > 0
    assert w.last_path == "fused" and w.last_gather is None        # (the last step's host tables are not pickled)


def test_driver_refusals(tmp_path, capsys):
    """--rnd_resized with --icarl_frames but without --resized_exemplars ends with the trainer's NotImplementedError (the driver
    reports a task's error with its traceback and stops there); --icarl_frames without an augmenting flag is a usage error."""
    from clsurvey_amd.framework import driver
    root = str(tmp_path)
    _friendly_base_model(root)
    flags = ["--rnd_resized", "4", "--icarl_frames"]
    driver.main(_common(root, *flags) + ["--method_name", "SI", "--runmode", "first_task_basemodel_dump"])
    capsys.readouterr()
    driver.main(_common(root, *flags) + ["--method_name", "ICARL"], method=_icarl())
    assert "NotImplementedError: icarl: exemplars are replayed with RandomCropFlip only" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="--icarl_frames belongs with"):
        driver.main(_common(str(tmp_path / "plain"), "--icarl_frames") + ["--method_name", "ICARL"], method=_icarl())
