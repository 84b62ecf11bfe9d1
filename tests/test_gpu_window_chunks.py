"""The crop and resized-crop window kernels where a channel plane takes MORE THAN ONE block: the twelve entries
clhip_{gather_tasks,rehearsal_assemble,icarl_assemble}_{crop_flip,resized_crop_flip}[_u8] at geometries whose launch plan, read out
of the library (clhip_resized_crop_plan, clhip_crop_rows_per_block) and asserted before use, splits the output lines into chunks.

Every resized-crop test elsewhere in the suite plans to ONE chunk (rpb == th), and outside the fp32 crop gather so does every crop
test, so y0 > 0, jlo = ylo[0] > 0, the band clamp against the plan's nb, an rpb set by the LDS limit, the rpb == 1 launch with more
than 48 KB of dynamic LDS, the refusal, and each caller's own decode of a block number into (row, channel, chunk) ran untested.

What is checked (outputs live in a kernel_parity.Arena of NaN sentinels with gaps, and gaps_untouched() follows every launch):
  * the fp32 resizing gather against the fp64 restatement (resized_crop_ref.restate) with ATen's fp32 CPU error on the same windows
    as the yardstick, the rule of test_gpu_resized_crop.py: e_kernel <= 4 e_ref, e_ref > 0; every window, every chunk
  * chunk invariance, bitwise: the same window content inside a second frame size whose plan has another rpb
  * the six resized entries bitwise equal on the same frames and windows (byte frames through a table holding -0.0, a denormal and
    an infinity), the assemblies with current rows, a ring row and >= 3 exemplars in ONE launch; identity windows bitwise the crop entry
  * bad rows between good ones, an output 4 bytes off a 16-byte boundary, the refusal (CLHIP_ENOTSUP, nothing written)
  * the six crop entries bitwise torch's indexing of the decoded frames at two and three chunks
Windows per resized geometry: 1 x 1 in two corners, the whole frame (= the largest accepted h and w at every geometry here) under
both flips, one window on each border, two identity windows (not at the enlargement), three draws of draw_resized_crop_flip.

PLANS as read from the library (rpb, chunks, nb, wmax, ktx, kty, lds_bytes), float / byte:
  (2, 80, 72, 70, 64)     (64, 2, 78, 72, 4, 4, 45248)   / (64, 2, 78, 72, 4, 4, 46272)    rpb = the 4096-element aim; 64 + 6 lines
  (2, 80, 80, 64, 64)     (64, 1, 80, 80, 4, 4, 48896)   / (59, 2, 78, 80, 4, 4, 48648)    one chunk against two
  (1, 100, 90, 72, 63)    (51, 2, 76, 90, 4, 4, 48996)   / (50, 2, 74, 90, 4, 4, 48772)    rpb set by the LDS; plain stores
  (2, 10, 12, 70, 64)     (64, 2, 10, 12, 3, 3, 5344)    / (64, 2, 10, 12, 3, 3, 6368)     enlargement, nb == Hs
  (1, 520, 300, 65, 40)   (2, 33, 27, 300, 16, 17, 39592) / (2, 33, 27, 300, 16, 17, 40616)  8x shrink in y, 17 taps
  (1, 512, 512, 64, 64)   (1, 64, 19, 512, 17, 17, 48460) / (1, 64, 19, 512, 17, 17, 49484)  rpb 1; the byte plan over 48 KB
  (1, 560, 560, 70, 70)   (1, 70, 19, 560, 17, 17, 52996) / (1, 70, 19, 560, 17, 17, 54020)  rpb 1; both plans over 48 KB
  (2, 160, 72, 70, 64)    (34, 3, 83, 72, 4, 6, 47520)   / (34, 3, 83, 72, 4, 6, 48544)    two planes of THREE chunks (see mutant d)
  (1, 530, 300, 65, 40)   the plan of 520 x 300 (bad rows: 521 lines fit the frame); (1, 40, 1100, 5, 140): CLHIP_ENOTSUP, both
  crop (lines per block, chunks): tw 64: 64, th 70 -> 2, th 130 -> 3; tw 63: 65, 2; tw 36: 113, 2; tw 4100: 1, 2

MEASURED on the MI355X (largest |result - fp64 restatement| over all windows; kernel, ATen fp32 CPU; then the range over the chunks).
Both share the fp32 rounding of the tap centres, which dominates: the two columns agree to three digits where a window is enlarged or
barely shrunk.
  geometry                 kernel      ATen        per chunk: kernel                ATen                     worst ratio in a chunk
  (2, 80, 72, 70, 64)      1.928e-05   1.928e-05   1.851e-05 (lines 64..69) .. 1.928e-05   the same            1.00
  (2, 80, 80, 64, 64)      3.466e-07   3.291e-07   one chunk                                                   1.05
  (1, 100, 90, 72, 63)     1.305e-05   1.305e-05   1.225e-05 .. 1.305e-05 (lines 51..71)   the same            1.00
  (2, 10, 12, 70, 64)      2.965e-06   2.965e-06   2.067e-06 (lines 64..69) .. 2.965e-06   the same            1.00
  (1, 520, 300, 65, 40)    4.319e-06   4.290e-06   9.940e-07 .. 4.319e-06 (chunk 32)       9.493e-07 .. 4.290e-06   1.05
  (1, 512, 512, 64, 64)    1.168e-07   1.187e-07   4.949e-08 .. 1.168e-07 (chunk 58)       5.349e-08 .. 1.187e-07   1.58
  (1, 560, 560, 70, 70)    4.124e-06   4.124e-06   1.335e-06 .. 4.124e-06 (chunk 61)       1.327e-06 .. 4.124e-06   1.03
  (2, 160, 72, 70, 64)     1.482e-05   1.482e-05   5.613e-06 (lines 0..33) .. 1.482e-05    5.617e-06 .. 1.482e-05   1.00
The second frame sizes of the invariance test (fp32 / u8): 80x85 / 80x82 (rpb 63), 80x81 (rpb 61, two chunks against one) / 80x82 (58),
100x91 (50) / 100x92 (49), 160x12 / 157x12 (63), 520x289 / 520x282 (rpb 3, 22 chunks), 512x356 / 512x349 (rpb 2, 32 chunks), 560x350 /
560x343 (rpb 2, 35 chunks), 160x77 / 160x74 (33).  No larger frame changes the plan of the 520, 512 and 560
frames (ratio and width are at their caps), so there the named frame is the larger one and the second frame its bottom right corner.
RUN TIME: 57 tests, 2.5 s for the file on the MI355X (the slowest test 0.3 s, which includes the first launch of the process).

NO BUG was found: all tests passed at the first complete run, the > 48 KB launches included, and tests/test_window_plan_cpu.py found no
window whose band or taps exceed the plan under any of its three evaluations of the tap formula.

MUTATION CHECK (run once with scratch builds of the library selected by CLHIP_LIB; nothing of it is kept; every mutant only reads
other in-bounds addresses).  Tests of this file that fail:
  (a) rz_resample_block: j0 = ylo[y] without - jlo (no effect when chunks == 1).  29: the restatement at every geometry but (2, 80, 80,
      64, 64); chunk invariance at all 14 cases; identity windows at 5 of 6; the family and infinity tests at the two geometries whose
      float and byte plans differ.  (Where all six entries share a plan they share the error: the family tests are no check of
      the block body, the restatement and the invariance are.)
  (b) rz_make_plan: nb two smaller.  The read-out sees it first: 36 tests fail at "no longer has the plan it was chosen for" (and
      test_window_plan_cpu.py fails: "a band of 5 lines", pinned plans).  With those asserts taken out of a scratch copy, 7 fail by
      value: restatement, invariance and family at (2, 80, 80, 64, 64) and (2, 10, 12, 70, 64), where the frame caps nb; elsewhere
      the plan's margin of 3 lines absorbs the 2.
  (c) the crop kernels: source line `top` instead of `top + y0` (no effect when chunks == 1).  8: the crop restatement at all 4
      geometries of that run (5 now), the crop bad rows, and identity windows at the 3 geometries whose crop launch takes two chunks,
      (2, 80, 72, 70, 64), (1, 100, 90, 72, 63) and (1, 560, 560, 70, 70).
  (d) rehearsal_assemble_rz_kernel: c = k % chunks (clamped below C), y0 from k / chunks.  First run: 11 (family and infinity at 5 of
      7 geometries, resized bad rows) and NONE at (2, 80, 72, 70, 64) and (2, 10, 12, 70, 64): with C == chunks == 2 the swapped decode
      visits the same (channel, chunk) pairs with the same results, an equivalent mutant there.  (2, 160, 72, 70, 64) and the crop
      geometry (2, 140, 72, 130, 64), two planes of three chunks, were added for that and carry the misaligned and the crop bad-row
      tests; second run: 14, the new geometry's family and infinity tests and the misaligned resized test among them.
"""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resized_crop_ref as ref  # noqa: E402
from kernel_parity import Arena, all_bits, bitwise_equal  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 4.0              # the rule of test_gpu_resized_crop.py: the kernel's error may be this many times ATen's fp32 CPU error
R = 8                     # CLHIP_RESIZE_MAX_RATIO
LDS_AIM = 48 * 1024
SENT = 0x7FC05A5A         # what every output float starts as: a NaN no kernel here can produce
LABEL_FILL = 99
B, N_OUT = 2, 12          # current rows of an assembly, width of iCaRL's target rows
ROW0, RING, SRC_IDX = 2, 1, [1]                                   # the ring run: frame 1 of the source goes to store row 2
INF_BYTE = 3              # the byte the table decodes to +inf; only _case(inf=True) stores it


# ---------------------------------------------------------------------------------------------- plans
def rz_plan(Hs, Ws, th, tw, byte):
    """(rpb, chunks, nb, wmax, ktx, kty, lds_bytes), or None where the entries refuse the frame."""
    import ctypes
    from clsurvey_amd import _lib
    out = (ctypes.c_int * 7)()
    rc = _lib.lib().clhip_resized_crop_plan(Hs, Ws, th, tw, int(byte), out)
    assert rc in (0, -3), rc
    return tuple(out) if rc == 0 else None


def cf_rows(tw):
    from clsurvey_amd import _lib
    return _lib.lib().clhip_crop_rows_per_block(tw)


# (C, Hs, Ws, th, tw) -> what the geometry is here for, as a predicate of (float plan, byte plan)
RESIZED = {
    (2, 80, 72, 70, 64): lambda f, b: f[:2] == (64, 2) and f[0] == cf_rows(64) and 70 - f[0] == 6 and b[1] == 2,
    (2, 80, 80, 64, 64): lambda f, b: f[:2] == (64, 1) and b[:2] == (59, 2),
    (1, 100, 90, 72, 63): lambda f, b: f[:2] == (51, 2) and b[:2] == (50, 2) and f[0] < min(72, cf_rows(63)) and 63 % 4 != 0,
    (2, 10, 12, 70, 64): lambda f, b: f[1] == 2 and b[1] == 2 and f[2] == 10 and b[2] == 10,
    (1, 520, 300, 65, 40): lambda f, b: f[:2] == (2, 33) and b[:2] == (2, 33) and f[5] == 17,
    (1, 512, 512, 64, 64): lambda f, b: f[:2] == (1, 64) and b[:2] == (1, 64) and b[6] > LDS_AIM >= f[6],
    (1, 560, 560, 70, 70): lambda f, b: f[:2] == (1, 70) and f[6] > LDS_AIM and b[6] > LDS_AIM,
    # two planes of THREE chunks (34 + 34 + 2 lines): where C == chunks, a decode that takes k % chunks for the channel and
    # k / chunks for the chunk visits the same (channel, chunk) pairs with the same results and cannot be seen
    (2, 160, 72, 70, 64): lambda f, b: f[:2] == (34, 3) and b[:2] == (34, 3),
}
RESIZED_GEOS = list(RESIZED)
BAD_RZ = (1, 530, 300, 65, 40)        # 521 lines are more than CLHIP_RESIZE_MAX_RATIO times 65 and fit the frame; 33 chunks
REFUSED = (1, 40, 1100, 5, 140)
CROP_GEOS = [(2, 72, 80, 70, 64), (1, 72, 80, 70, 63), (1, 140, 40, 130, 36), (1, 5, 4200, 2, 4100), (2, 140, 72, 130, 64)]
CROP_PLAN = {(70, 64): (64, 2), (70, 63): (65, 2), (130, 36): (113, 2), (2, 4100): (1, 2), (130, 64): (64, 3)}      # (th, tw) -> (rpb, chunks)


def _ids(geos):
    return ["%dx%dx%d_to_%dx%d" % g for g in geos]


def _assert_resized_property(geo):
    f, b = rz_plan(*geo[1:], False), rz_plan(*geo[1:], True)
    assert f is not None and b is not None, (geo, f, b)
    assert RESIZED[geo](f, b), "%r no longer has the plan it was chosen for: float %r, byte %r" % (geo, f, b)
    return f, b


def _assert_crop_property(geo):
    C, Hs, Ws, th, tw = geo
    rpb = cf_rows(tw)
    assert (rpb, (th + rpb - 1) // rpb) == CROP_PLAN[(th, tw)], "%r no longer takes its chunks: %d lines per block" % (geo, rpb)
    return rpb


# ---------------------------------------------------------------------------------------------- frames, windows, launches
def _lut(C, gen):
    """fp32 [C][256]: random values with -0.0, a denormal and an infinity among them."""
    lut = torch.randn((C, 256), generator=gen)
    lut[:, 0], lut[:, 1] = 0.0, -0.0
    lut[:, 2] = torch.tensor([1], dtype=torch.int32).view(torch.float32)
    lut[:, INF_BYTE] = float("inf")
    return lut


def _decode(fb, lut):
    """What byte frames mean: lut[c][v] (indexing, no arithmetic)."""
    return torch.stack([lut[c][fb[:, c].long()] for c in range(fb.shape[1])], 1)


def _make_case(geo, fb, lut, gen):
    """fb: uint8 [3][C][Hs][Ws].  The fp32 entries run on the decoded frames.  Nothing here is written to by a launch (the
    rehearsal launches work on a clone of the store)."""
    C, Hs, Ws, th, tw = geo
    assert tuple(fb.shape) == (3, C, Hs, Ws) and C <= 2
    c = types.SimpleNamespace(geo=geo, fb=fb, lut=lut, dec=_decode(fb, lut), x=torch.randn((B, C, th, tw), generator=gen),
                              y=torch.randint(1, 20, (B,), generator=gen), store_y=torch.tensor([11, 12, 13]),
                              store_t=torch.randn((3, N_OUT), generator=gen))
    for k in ("fb", "lut", "dec", "x", "y", "store_y", "store_t"):
        setattr(c, k + "_dev", getattr(c, k).to(DEV))
    return c


@functools.lru_cache(maxsize=None)
def _case(geo, inf=False):
    C, Hs, Ws, th, tw = geo
    gen = torch.Generator().manual_seed(7 * Hs + 3 * Ws + th + int(inf))
    fb = torch.randint(0, 256, (3, C, Hs, Ws), generator=gen, dtype=torch.uint8)
    fb[fb == INF_BYTE] = INF_BYTE + 1
    fb[0, 0, 0, 0], fb[0, 0, Hs - 1, Ws - 1], fb[1, C - 1, Hs // 2, Ws // 2] = 1, 2, 1       # -0.0 and the denormal are there
    if inf:
        fb[0, 0, Hs // 3, Ws // 3], fb[1, C - 1, Hs - 1, 0] = INF_BYTE, INF_BYTE
    return _make_case(geo, fb, _lut(C, gen), gen)


def _windows(Hs, Ws, th, tw, drawn=3):
    """1 x 1 in two corners; the largest accepted window (the whole frame where it is accepted) under both flips, at both ends;
    one window on each border; identity windows (h == th, w == tw; an odd left, and the far corner) where the frame has room; and
    a few draws of the default RandomResizedCropFlip.  Rows of (top, left, h, w, flip)."""
    from clsurvey_amd.data import RandomResizedCropFlip, draw_resized_crop_flip
    hm, wm = min(Hs, R * th), min(Ws, R * tw)
    h, w = max(1, (2 * hm) // 3), max(1, (2 * wm) // 3)
    wins = [[0, 0, 1, 1, 0], [Hs - 1, Ws - 1, 1, 1, 1], [Hs - hm, Ws - wm, hm, wm, 0], [0, 0, hm, wm, 1],
            [0, (Ws - w) // 2, h, w, 1], [Hs - h, (Ws - w) // 2, h, w, 0], [(Hs - h) // 2, 0, h, w, 1], [(Hs - h) // 2, Ws - w, h, w, 0]]
    if th <= Hs and tw <= Ws:
        wins += [[(Hs - th) // 2, min(Ws - tw, ((Ws - tw) // 2) | 1), th, tw, 0], [Hs - th, Ws - tw, th, tw, 1]]
    if drawn and Hs <= R * th and Ws <= R * tw:
        gen = torch.Generator().manual_seed(Hs + 2 * tw)
        wins += draw_resized_crop_flip(drawn, RandomResizedCropFlip((th, tw)), (Hs, Ws), gen).tolist()
    for top, left, hh, ww, flip in wins:
        assert 0 <= top <= Hs - hh and 0 <= left <= Ws - ww and 1 <= hh <= hm and 1 <= ww <= wm and flip in (0, 1)
    return wins


def _crop_windows(Hs, Ws, th, tw):
    """Every corner position under both flips, and an odd left under both.  Rows of (top, left, flip)."""
    mt, ml = Hs - th, Ws - tw
    odd = min(ml, (ml // 2) | 1)
    return [[0, 0, 0], [0, ml, 1], [mt, 0, 1], [mt, ml, 0], [0, 0, 1], [0, ml, 0], [mt, 0, 0], [mt, ml, 1], [mt // 2, odd, 0],
            [min(1, mt), odd, 1]]


def _outs(sizes, misaligned=False):
    """Output tensors of `sizes` floats in one Arena, all SENT, with sentinel gaps between them: (arena, keys, device views)."""
    a = Arena()
    keys = [a.add(n, misaligned=misaligned, fill=SENT) for n in sizes]
    a.upload(DEV)
    views = [a.dev[a.items[k][0]:a.items[k][0] + n] for k, n in zip(keys, sizes)]
    assert all(v.data_ptr() % 16 == (4 if misaligned else 0) for v in views)
    return a, keys, views


def _back(a, keys):
    torch.cuda.synchronize()
    a.download()
    assert a.gaps_untouched(), "a write outside the outputs"
    return [a.get(k) for k in keys]


def _labels(n):
    return torch.full((n + 4,), LABEL_FILL, dtype=torch.int64, device=DEV)


def _labels_back(lab, n):
    host = lab.cpu()
    assert host[:2].tolist() == [LABEL_FILL] * 2 and host[n + 2:].tolist() == [LABEL_FILL] * 2, "a write outside the labels"
    return host[2:n + 2]


def _call(fn, expect):
    from clsurvey_amd import _lib
    if expect is None:
        fn()
    else:
        with pytest.raises(_lib.ClhipError, match=expect):
            fn()


def _i32(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV).contiguous()


def _name(family, resized, byte):
    return "%s_%scrop_flip%s" % (family, "resized_" if resized else "", "_u8" if byte else "")


def gather(c, resized, byte, rows, params, misaligned=False, expect=None):
    """clhip_gather_tasks_[resized_]crop_flip[_u8] over a one-task table laid over the frames: (x [n][C][th][tw], labels [n])."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = c.geo
    frames = c.fb_dev if byte else c.dec_dev
    table = ops.task_table([frames], [c.store_y_dev], [frames.shape[0]], [0], DEV)
    n = len(rows)
    a, keys, (xv,) = _outs([n * C * th * tw], misaligned)
    lab = _labels(n)
    args = (table, c.geo) + ((c.lut_dev,) if byte else ()) + (torch.tensor(rows, device=DEV), _i32(params))
    _call(lambda: getattr(ops, _name("gather_tasks", resized, byte))(*args, x_out=xv, labels_out=lab[2:2 + n]), expect)
    (x,) = _back(a, keys)
    return x.view(n, C, th, tw), _labels_back(lab, n)


def rehearsal(c, resized, byte, rows, params, misaligned=False, expect=None):
    """clhip_rehearsal_assemble_[resized_]crop_flip[_u8] with all three runs: B current rows, one ring row (source frame 1 ->
    store row 2), the exemplar rows.  (x_mix [B + E][C][th][tw], labels_mix, store, store labels)."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = c.geo
    frames = c.fb_dev if byte else c.dec_dev
    store, store_y = frames.clone(), c.store_y_dev.clone()
    store[ROW0] = 0
    assert all(0 <= r < ROW0 or r >= 3 or r < 0 for r in rows), "an exemplar row must not be a ring row of the same launch"
    n = B + len(rows)
    a, keys, (xv,) = _outs([n * C * th * tw], misaligned)
    lab = _labels(n)
    table = (c.lut_dev,) if byte else ()
    _call(lambda: getattr(ops, _name("rehearsal_assemble", resized, byte))(
        c.geo, *table, c.x_dev, c.y_dev, B, frames, torch.tensor(SRC_IDX, device=DEV), store, store_y, ROW0, RING, _i32(rows),
        _i32(params), xv, lab[2:2 + n]), expect)
    (x,) = _back(a, keys)
    return x.view(n, C, th, tw), _labels_back(lab, n), store.cpu(), store_y.cpu()


def icarl(c, resized, byte, rows, params, misaligned=False, expect=None):
    """clhip_icarl_assemble_[resized_]crop_flip[_u8] with all three runs: (x_mix, labels_mix, t_mix [B + E][N_OUT])."""
    from clsurvey_amd import ops
    C, Hs, Ws, th, tw = c.geo
    n = B + len(rows)
    a, keys, (xv, tv) = _outs([n * C * th * tw, n * N_OUT], misaligned)
    lab = _labels(n)
    table = (c.lut_dev,) if byte else ()
    _call(lambda: getattr(ops, _name("icarl_assemble", resized, byte))(
        c.geo, *table, c.x_dev, c.y_dev, B, c.fb_dev if byte else c.dec_dev, _i32(rows), _i32(params), c.store_t_dev, xv,
        lab[2:2 + n], tv.view(n, N_OUT)), expect)
    x, t = _back(a, keys)
    return x.view(n, C, th, tw), _labels_back(lab, n), t.view(n, N_OUT)


def _frame_rows(n):
    return [k % ROW0 for k in range(n)]                             # frames 0 and 1 in turn: never the ring row


def check_rehearsal(c, byte, got, rows, want_x, bad=()):
    """The restatement of test_gpu_exemplar_resized.py: the current rows and their labels are the inputs, the ring row and its
    store label are the source frame and the batch label, the rest of the store is untouched, the exemplar rows are `want_x` with
    the stored labels; rows in `bad` keep the sentinel and get label -1."""
    x_mix, y_mix, store, store_y = got
    frames = c.fb if byte else c.dec
    assert bitwise_equal(x_mix[:B], c.x) and torch.equal(y_mix[:B], c.y)
    assert torch.equal(store[:ROW0].view(-1).view(torch.uint8), frames[:ROW0].reshape(-1).view(torch.uint8))
    assert torch.equal(store[ROW0].view(-1).view(torch.uint8), frames[SRC_IDX[0]].reshape(-1).view(torch.uint8))
    assert store_y.tolist() == c.store_y[:ROW0].tolist() + [int(c.y[0])]
    for e, g in enumerate(rows):
        if e in bad:
            assert all_bits(x_mix[B + e], SENT) and int(y_mix[B + e]) == -1, "bad row %d" % e
        else:
            assert bitwise_equal(x_mix[B + e], want_x[e]), "exemplar row %d" % e
            assert int(y_mix[B + e]) == int(c.store_y[g])


def check_icarl(c, got, rows, want_x, bad=()):
    """The restatement of test_gpu_icarl_augment.py: current rows and labels are the inputs, the exemplar rows are `want_x` with
    label 0 and the stored target row; the current rows' targets are not written; rows in `bad` keep the sentinel in x_mix AND in
    t_mix and get label -1."""
    x_mix, y_mix, t_mix = got
    assert bitwise_equal(x_mix[:B], c.x) and torch.equal(y_mix[:B], c.y) and all_bits(t_mix[:B], SENT)
    for e, g in enumerate(rows):
        if e in bad:
            assert all_bits(x_mix[B + e], SENT) and all_bits(t_mix[B + e], SENT) and int(y_mix[B + e]) == -1, "bad row %d" % e
        else:
            assert bitwise_equal(x_mix[B + e], want_x[e]), "exemplar row %d" % e
            assert int(y_mix[B + e]) == 0 and bitwise_equal(t_mix[B + e], c.store_t[g])


def check_family(c, resized, rows, params, want_x, bad=(), misaligned=False, skip_anchor=False):
    """Every entry of the family (skip_anchor: all but the fp32 gather, which made `want_x`) on the same frames and windows:
    bitwise `want_x`."""
    for byte in (False, True):
        if byte or not skip_anchor:
            x, y = gather(c, resized, byte, rows, params, misaligned)
            for e, g in enumerate(rows):
                if e in bad:
                    assert all_bits(x[e], SENT) and int(y[e]) == -1, "bad row %d" % e
                else:
                    assert bitwise_equal(x[e], want_x[e]), "gather%s row %d" % ("_u8" if byte else "", e)
                    assert int(y[e]) == int(c.store_y[g])
        check_rehearsal(c, byte, rehearsal(c, resized, byte, rows, params, misaligned), rows, want_x, bad)
        check_icarl(c, icarl(c, resized, byte, rows, params, misaligned), rows, want_x, bad)


def _groups(n, most=10):
    """Slices of 0 .. n in launches of nearly equal size, at most 10 exemplar rows each beside the B current rows: 12 rows a launch."""
    k = (n + most - 1) // most
    cuts = [n * j // k for j in range(k + 1)]
    return [slice(a, b) for a, b in zip(cuts, cuts[1:])]


@functools.lru_cache(maxsize=None)
def _anchor(geo):
    """The fp32 gather over every window of the geometry, once: (rows, windows, x [n][C][th][tw])."""
    c = _case(geo)
    wins = _windows(*geo[1:])
    rows = _frame_rows(len(wins))
    xs = []
    for s in _groups(len(wins)):
        x, y = gather(c, True, False, rows[s], wins[s])
        assert y.tolist() == [int(c.store_y[g]) for g in rows[s]]
        xs.append(x)
    return rows, wins, torch.cat(xs)


# ---------------------------------------------------------------------------------------------- resized crop
@pytest.mark.parametrize("geo", RESIZED_GEOS, ids=_ids(RESIZED_GEOS))
def test_resized_gather_is_the_restatement_within_atens_own_error_in_every_chunk(geo):
    """e_ref = ATen's fp32 CPU error against the fp64 restatement over all windows of the geometry; the kernel's error over the
    same windows is at most MARGIN e_ref.  No window and no chunk is left out; the figures are printed per chunk."""
    f, b = _assert_resized_property(geo)
    C, Hs, Ws, th, tw = geo
    c = _case(geo)
    rows, wins, x = _anchor(geo)
    idx, params = torch.tensor(rows), torch.tensor(wins, dtype=torch.int32)
    want = ref.restate(c.dec, idx, params, th, tw)
    aten = ref.aten(c.dec, idx, params, th, tw)
    assert bool(torch.isfinite(want).all()) and tuple(want.shape) == tuple(x.shape)
    d_kernel, d_ref = (x.double() - want).abs(), (aten.double() - want).abs()
    rpb, chunks = f[:2]
    worst = (0.0, 0.0, 0)
    for k in range(chunks):
        lines = slice(k * rpb, min(th, (k + 1) * rpb))
        ek, er = float(d_kernel[:, :, lines].max()), float(d_ref[:, :, lines].max())
        print("MEASURED|%s|chunk %d of %d, lines %d..%d|%.3e|%.3e" % (_ids([geo])[0], k, chunks, lines.start, lines.stop - 1, ek, er))
        worst = max(worst, (ek, er, k))
    e_kernel, e_ref = float(d_kernel.max()), float(d_ref.max())
    print("MEASURED|%s|all %d chunks (worst chunk %d)|%.3e|%.3e" % (_ids([geo])[0], chunks, worst[2], e_kernel, e_ref))
    assert e_ref > 0.0
    assert e_kernel <= MARGIN * e_ref


@pytest.mark.parametrize("geo", RESIZED_GEOS, ids=_ids(RESIZED_GEOS))
def test_six_resized_entries_are_bitwise_equal_with_all_three_runs_in_a_launch(geo):
    """The byte gather and the four assemblies against the fp32 gather, on the same frames and windows.  The assemblies carry
    B = 2 current rows and a ring row in front of their exemplar run, so an exemplar block's number decodes to every (exemplar,
    channel, chunk); current rows, ring row, store labels and iCaRL's targets are the restatements of check_rehearsal /
    check_icarl."""
    f, b = _assert_resized_property(geo)
    assert max(f[1], b[1]) > 1                                                      # crop_blocks = C chunks > C
    rows, wins, x = _anchor(geo)
    for s in _groups(len(wins)):
        assert s.stop - s.start >= 3                                                # E >= 3 exemplars behind the copy and ring blocks
        check_family(_case(geo), True, rows[s], wins[s], x[s], skip_anchor=True)


@pytest.mark.parametrize("geo", RESIZED_GEOS, ids=_ids(RESIZED_GEOS))
def test_six_resized_entries_agree_on_minus_zero_a_denormal_and_an_infinity(geo):
    """Frames that hold the byte decoded to +inf: a tap of weight 0 takes no part, every other one gives +inf, in all six entries
    alike (no tolerance; nothing is compared with the restatement)."""
    _assert_resized_property(geo)
    C, Hs, Ws, th, tw = geo
    c = _case(geo, inf=True)
    wins = _windows(Hs, Ws, th, tw, drawn=0)[2:6] + [[Hs // 3, Ws // 3, 1, 1, 0]]
    rows = [0, 1, 0, 1, 0]
    x, _ = gather(c, True, False, rows, wins)
    assert bool(torch.isinf(x).any()) and not bool(torch.isnan(x).any()) and bool(torch.isinf(x[4, 0]).all())
    check_family(c, True, rows, wins, x, skip_anchor=True)


def _other_frame(geo, byte):
    """A second frame size (Hs2, Ws2) whose plan for the same output has another rpb: the frame widened, else heightened, until
    the read-out says so; where no larger frame changes the plan (the ratio and the width are at their caps), narrowed, else
    shortened."""
    C, Hs, Ws, th, tw = geo
    rpb = rz_plan(Hs, Ws, th, tw, byte)[0]
    tries = ([(Hs, w) for w in range(Ws + 1, Ws + 257)] + [(h, Ws) for h in range(Hs + 1, Hs + 257)] +
             [(Hs, w) for w in range(Ws - 1, 0, -1)] + [(h, Ws) for h in range(Hs - 1, 0, -1)])
    for h2, w2 in tries:
        p = rz_plan(h2, w2, th, tw, byte)
        if p is not None and p[0] != rpb:
            return h2, w2, p
    raise AssertionError("no frame size with another rpb for %r" % (geo,))


@pytest.mark.parametrize("byte", [False, True], ids=["fp32", "u8"])
@pytest.mark.parametrize("geo", RESIZED_GEOS, ids=_ids(RESIZED_GEOS))
def test_the_result_does_not_depend_on_the_chunking(geo, byte):
    """Taps and summation order depend on (h, w, th, tw, flip, o) alone, never on the plan: the same window content inside a second
    frame size whose plan has another rpb gives the same bits.  The smaller of the two frames is the bottom right corner of the
    larger one; the windows are those of the smaller frame.  Any error at a chunk boundary fails this, without a tolerance."""
    plans = _assert_resized_property(geo)
    C, Hs, Ws, th, tw = geo
    h2, w2, p2 = _other_frame(geo, byte)
    assert p2[0] != plans[int(byte)][0] and max(p2[1], plans[int(byte)][1]) > 1
    print("MEASURED|%s|%s|rpb %d, %d chunks|other frame %dx%d: rpb %d, %d chunks" % (
        _ids([geo])[0], "u8" if byte else "fp32", plans[int(byte)][0], plans[int(byte)][1], h2, w2, p2[0], p2[1]))
    c = _case(geo)
    if h2 >= Hs and w2 >= Ws:                                       # the named frame inside a larger one
        gen = torch.Generator().manual_seed(h2 + w2)
        fb = torch.randint(0, 256, (3, C, h2, w2), generator=gen, dtype=torch.uint8)
        fb[fb == INF_BYTE] = INF_BYTE + 1
        fb[:, :, h2 - Hs:, w2 - Ws:] = c.fb
        small, big = c, _make_case((C, h2, w2, th, tw), fb, c.lut, gen)
    else:                                                           # a smaller one inside the named frame
        gen = torch.Generator().manual_seed(h2 + w2)
        small, big = _make_case((C, h2, w2, th, tw), c.fb[:, :, Hs - h2:, Ws - w2:].contiguous(), c.lut, gen), c
    dy, dx = big.geo[1] - small.geo[1], big.geo[2] - small.geo[2]
    assert dy >= 0 and dx >= 0 and dy + dx > 0
    wins = _windows(small.geo[1], small.geo[2], th, tw)
    rows = _frame_rows(len(wins))
    for s in _groups(len(wins)):
        xs, ys = gather(small, True, byte, rows[s], wins[s])
        xb, yb = gather(big, True, byte, rows[s], [[t + dy, l + dx, h, w, f] for t, l, h, w, f in wins[s]])
        for e, win in enumerate(wins[s]):
            assert bitwise_equal(xs[e], xb[e]), "window %r" % (win,)
        assert torch.equal(ys, yb)


IDENTITY_GEOS = [g for g in RESIZED_GEOS if g[3] <= g[1] and g[4] <= g[2]]


@pytest.mark.parametrize("geo", IDENTITY_GEOS, ids=_ids(IDENTITY_GEOS))
def test_identity_windows_are_the_crop_entry_bitwise(geo):
    """h == th and w == tw: one tap of weight exactly 1 per axis in every chunk, so the rows are those of
    clhip_gather_tasks_crop_flip for (top, left, flip)."""
    _assert_resized_property(geo)
    assert len(IDENTITY_GEOS) == len(RESIZED_GEOS) - 1              # all but the enlargement, which has no such window
    C, Hs, Ws, th, tw = geo
    rows, wins, x = _anchor(geo)
    ident = [k for k, w in enumerate(wins) if w[2] == th and w[3] == tw]
    assert len(ident) >= 2
    want, _ = gather(_case(geo), False, False, [rows[k] for k in ident], [[wins[k][0], wins[k][1], wins[k][4]] for k in ident])
    for e, k in enumerate(ident):
        assert bitwise_equal(x[k], want[e])


def _crop_restate(c, rows, params):
    """torchvision's crop, then hflip, of the decoded frames, by indexing."""
    C, Hs, Ws, th, tw = c.geo
    out = [c.dec[g, :, top:top + th, left:left + tw] for g, (top, left, _) in zip(rows, params)]
    return torch.stack([v.flip(-1) if p[2] else v for v, p in zip(out, params)])


@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized"])
def test_bad_rows_between_good_ones_keep_the_sentinel_in_every_chunk(resized):
    """A gather index one past the frames, a window past the bottom edge, and (resized) h one over CLHIP_RESIZE_MAX_RATIO th inside
    the frame, each between good rows, in all six entries: the bad rows keep the sentinel in all their lines and get label -1 (in
    iCaRL's assembly their target rows keep it too), the good rows are what a launch of the good rows alone gives."""
    if resized:
        geo = BAD_RZ
        f, b = rz_plan(*geo[1:], False), rz_plan(*geo[1:], True)
        assert f[1] == 33 and b[1] == 33 and geo[1] > R * geo[3]
        good = _windows(*geo[1:], drawn=0)[2:6]
        bad_params = [good[0], [geo[1] - 10, 0, 11, 20, 0], [3, 0, R * geo[3] + 1, 100, 0]]
        assert 3 + R * geo[3] + 1 <= geo[1]
    else:
        geo = CROP_GEOS[-1]
        _assert_crop_property(geo)
        good = _crop_windows(*geo[1:])[:4]
        bad_params = [good[0], [geo[1] - geo[3] + 1, 0, 0]]
    c = _case(geo)
    rows = [0, 3, 1, 0, 1, 1, 0][:2 * len(bad_params) + 1]
    params = [good[0], bad_params[0], good[1], bad_params[1], good[2]] + ([bad_params[2], good[3]] if resized else [])
    bad = tuple(range(1, len(rows), 2))
    keep = [k for k in range(len(rows)) if k not in bad]
    alone, _ = gather(c, resized, False, [rows[k] for k in keep], [params[k] for k in keep])
    if not resized:
        assert bitwise_equal(alone, _crop_restate(c, [rows[k] for k in keep], [params[k] for k in keep]))
    want = [None] * len(rows)
    for e, k in enumerate(keep):
        want[k] = alone[e]
    check_family(c, resized, rows, params, want, bad=bad)


@pytest.mark.parametrize("resized", [False, True], ids=["crop", "resized"])
def test_an_output_four_bytes_off_takes_the_plain_stores_and_gives_the_same_bits(resized):
    """tw % 4 == 0, two planes of three chunks, and every output (x_out, x_mix, t_mix) one float past a 16-byte boundary: all six
    entries."""
    geo = RESIZED_GEOS[-1] if resized else CROP_GEOS[-1]
    assert geo[0] == 2
    if resized:
        _assert_resized_property(geo)
        rows, wins, x = _anchor(geo)
        rows, wins, x = rows[:8], wins[:8], x[:8]
    else:
        _assert_crop_property(geo)
        wins = _crop_windows(*geo[1:])[:8]
        rows = _frame_rows(8)
        x, _ = gather(_case(geo), False, False, rows, wins)
    assert geo[4] % 4 == 0
    check_family(_case(geo), resized, rows, wins, x, misaligned=True)


def test_a_frame_without_a_plan_is_enotsup_from_all_six_resized_entries():
    """One output line's band of 40 x 1100 -> 5 x 140 does not fit 64 KB: nothing is launched, every output keeps its sentinel,
    the store its rows."""
    geo = REFUSED
    assert rz_plan(*geo[1:], False) is None and rz_plan(*geo[1:], True) is None
    c = _case(geo)
    rows, wins = [0, 1, 0], [[0, 0, 40, 1100, 0], [3, 7, 20, 600, 1], [0, 0, 5, 140, 0]]
    for byte in (False, True):
        x, y = gather(c, True, byte, rows, wins, expect="CLHIP_ENOTSUP")
        assert all_bits(x, SENT) and y.tolist() == [LABEL_FILL] * 3
        x, y, store, store_y = rehearsal(c, True, byte, rows, wins, expect="CLHIP_ENOTSUP")
        assert all_bits(x, SENT) and y.tolist() == [LABEL_FILL] * (B + 3) and store_y.tolist() == c.store_y.tolist()
        assert not bool(store[ROW0].any()) and torch.equal(store[:ROW0], (c.fb if byte else c.dec)[:ROW0])
        x, y, t = icarl(c, True, byte, rows, wins, expect="CLHIP_ENOTSUP")
        assert all_bits(x, SENT) and all_bits(t, SENT) and y.tolist() == [LABEL_FILL] * (B + 3)


# ---------------------------------------------------------------------------------------------- crop
@pytest.mark.parametrize("geo", CROP_GEOS, ids=_ids(CROP_GEOS))
def test_six_crop_entries_are_the_indexing_restatement_in_both_chunks(geo):
    """Two chunks of 64 + 6 lines / the same with plain stores (tw = 63) / 113 + 17 lines / one line per block (tw >= 4096) / two
    planes of three chunks (64 + 64 + 2 lines: a k -> (c, y0) decode with the roles swapped is no permutation there).  Both
    flips at every corner position and an odd left.  The fp32 gather (the anchor) and the five entries with a k -> (c, y0) decode
    of their own are bitwise torch's indexing of the decoded frames."""
    _assert_crop_property(geo)
    c = _case(geo)
    wins = _crop_windows(*geo[1:])
    rows = _frame_rows(len(wins))
    check_family(c, False, rows, wins, _crop_restate(c, rows, wins))
