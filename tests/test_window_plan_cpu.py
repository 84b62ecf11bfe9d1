"""The launch plans of the window entries, read out on the host (clhip_resized_crop_plan, clhip_crop_rows_per_block of
include/clhip.h) and checked without a GPU: the split of a channel plane into chunks, the LDS limits, the byte entries' table, the
LDS layout of rz_resample_block (csrc/resized_crop.hpp) against the plan's bytes, and that the plan's band (nb lines) and tap counts
(ktx, kty) hold every window the kernels accept, in every chunk, for the tap formula of clhip.h evaluated three ways: float32
operation by operation (numpy), float64, and float32 with the product scale * (o + 0.5) kept exact into the following add (what
a device fused multiply-add does).  Per output line the smallest lo and the largest hi of the three are taken.

The grid: every (Hs, th) of 1..140 + {256, 300, 512, 520, 1100} x 1..80 + {130, 140, 224} under a handful of (Ws, tw), and every
(Ws, tw) of the same ranges under a handful of (Hs, th), both element types.  The tap tables depend on (window extent, output
extent) alone and are made once per output extent."""
import ctypes as C
import functools

import numpy as np
import pytest

R = 8                                    # CLHIP_RESIZE_MAX_RATIO
LDS_AIM, LDS_MAX, LUT_BYTES = 48 * 1024, 64 * 1024, 1024
EINVAL, ENOTSUP = -1, -3
INS = list(range(1, 141)) + [256, 300, 512, 520, 1100]
OUTS = list(range(1, 81)) + [130, 140, 224]
SIDE_WIDTHS = [(1, 1), (7, 8), (64, 64), (72, 63), (139, 4), (300, 40), (512, 64), (1100, 140)]       # (Ws, tw) under every (Hs, th)
SIDE_HEIGHTS = [(1, 1), (5, 8), (64, 56), (100, 72), (140, 3), (256, 224), (520, 65), (1100, 130)]    # (Hs, th) under every (Ws, tw)


def plan(Hs, Ws, th, tw, byte):
    """(rc, (rpb, chunks, nb, wmax, ktx, kty, lds_bytes)) as the library reads it out."""
    from clsurvey_amd import _lib
    out = (C.c_int * 7)(*([-99] * 7))
    rc = _lib.lib().clhip_resized_crop_plan(Hs, Ws, th, tw, int(byte), out)
    return rc, tuple(out)


@functools.lru_cache(maxsize=None)
def tap_tables(n_out):
    """For every window extent n in 1 .. min(1100, R n_out) (row n - 1) and output element o: lo [n][o] (the smallest of the
    three evaluations), hi [n][o] (the largest; before the kernel's lo + KT clamp), and the taps the block body derives for the
    window, ceilf(2 max(n / n_out, 1)) + 1 in float32."""
    n_max = min(max(INS), R * n_out)
    n = np.arange(1, n_max + 1, dtype=np.int64)[:, None]
    o = np.arange(n_out, dtype=np.int64)[None, :]
    f32 = np.float32
    scale = n.astype(f32) / f32(n_out)
    sup = np.maximum(scale, f32(1))
    t = o.astype(f32) + f32(0.5)
    los, his = [], []
    # float32, operation by operation
    c = scale * t
    los.append((c - sup + f32(0.5)).astype(np.int64))
    his.append((c + sup + f32(0.5)).astype(np.int64))
    assert c.dtype == np.float32 and (c - sup + f32(0.5)).dtype == np.float32
    # float32 with the product exact into the add (both fit float64 without rounding), then + 0.5f in float32
    prod = scale.astype(np.float64) * t.astype(np.float64)
    los.append(((prod - sup).astype(f32) + f32(0.5)).astype(np.int64))
    his.append(((prod + sup).astype(f32) + f32(0.5)).astype(np.int64))
    # float64 from the integers
    s64 = n.astype(np.float64) / float(n_out)
    u64 = np.maximum(s64, 1.0)
    c64 = s64 * (o.astype(np.float64) + 0.5)
    los.append((c64 - u64 + 0.5).astype(np.int64))
    his.append((c64 + u64 + 0.5).astype(np.int64))
    lo = np.minimum(np.maximum(0, np.minimum.reduce(los)), n - 1)                   # (astype truncates towards zero, as the C cast)
    hi = np.maximum(np.minimum(n, np.maximum.reduce(his)), lo + 1)
    kt_body = (np.ceil(f32(2) * np.maximum(n[:, 0].astype(f32) / f32(n_out), f32(1))).astype(np.int64) + 1)
    return lo, hi, kt_body


@functools.lru_cache(maxsize=None)
def widest_support(n_out):
    """prefix[n - 1] = the most taps hi - lo of any output element over the window extents 1 .. n.  Also asserts, once per output
    extent, that no window needs more taps than the block body derives for it."""
    lo, hi, kt_body = tap_tables(n_out)
    support = (hi - lo).max(axis=1)
    over = np.nonzero(support > kt_body)[0]
    assert over.size == 0, "window extent %d -> %d: %d taps, the block body derives %d" % (over[0] + 1, n_out, support[over[0]], kt_body[over[0]])
    return np.maximum.accumulate(support)


@functools.lru_cache(maxsize=None)
def widest_band(n_out, rpb):
    """prefix[n - 1] = the most source lines hi(last line) - lo(first line) of any chunk y0 = 0, rpb, ... over the window extents
    1 .. n."""
    lo, hi, _ = tap_tables(n_out)
    first = np.arange(0, n_out, rpb)
    last = np.minimum(first + rpb, n_out) - 1
    return np.maximum.accumulate((hi[:, last] - lo[:, first]).max(axis=1))


def check_geometry(Hs, Ws, th, tw):
    """Both element types of one geometry.  Returns the two (rc, plan)."""
    res = []
    for byte in (False, True):
        rc, p = plan(Hs, Ws, th, tw, byte)
        res.append((rc, p))
        what = "%dx%d -> %dx%d %s: %r" % (Hs, Ws, th, tw, "u8" if byte else "f32", p)
        if rc != 0:
            assert rc == ENOTSUP and p == (-99,) * 7, what
            continue
        rpb, chunks, nb, wmax, ktx, kty, lds = p
        assert 1 <= rpb <= th and chunks * rpb >= th > (chunks - 1) * rpb, what
        assert lds <= LDS_MAX and (lds <= LDS_AIM or rpb == 1), what
        assert 1 <= nb <= Hs and wmax == min(Ws, R * tw), what
        # the LDS rz_resample_block lays out: raw [nb][wmax] (rounded up to 4 floats), tmp [nb][tw], wx [ktx][tw], wy [kty][rpb], xlo
        # [tw], ylo [rpb], yhi [rpb], and the byte entries' table
        floats = (nb * wmax + 3) // 4 * 4 + nb * tw + ktx * tw + kty * rpb + tw + 2 * rpb
        assert lds == 4 * floats + (LUT_BYTES if byte else 0), what
        # every accepted window, 1 <= h <= min(Hs, R th) and 1 <= w <= min(Ws, R tw), in every chunk
        h_max, w_max = min(Hs, R * th), min(Ws, R * tw)
        assert widest_support(th)[h_max - 1] <= kty, what + ": %d vertical taps" % widest_support(th)[h_max - 1]
        assert widest_support(tw)[w_max - 1] <= ktx, what + ": %d horizontal taps" % widest_support(tw)[w_max - 1]
        assert widest_band(th, rpb)[h_max - 1] <= nb, what + ": a band of %d lines" % widest_band(th, rpb)[h_max - 1]
    (rf, pf), (rb, pb) = res
    if rf != 0:
        assert rb != 0, "the byte plan needs more than the float plan: %r" % (res,)
    if rf == 0 and rb == 0:
        assert pb[0] <= pf[0]
        if pb[0] == pf[0]:
            assert pb[:6] == pf[:6] and pb[6] == pf[6] + LUT_BYTES, res
    return res


def test_vertical_axis_of_the_grid():
    served = refused = multi = 0
    for Ws, tw in SIDE_WIDTHS:
        for Hs in INS:
            for th in OUTS:
                for rc, p in check_geometry(Hs, Ws, th, tw):
                    served += rc == 0
                    refused += rc != 0
                    multi += rc == 0 and p[1] > 1
    print("vertical grid: %d plans, %d of them with more than one chunk, %d refusals" % (served, multi, refused))
    assert served > 10000 and multi > 1000 and refused > 0


def test_horizontal_axis_of_the_grid():
    served = refused = limited = 0
    for Hs, th in SIDE_HEIGHTS:
        for Ws in INS:
            for tw in OUTS:
                for rc, p in check_geometry(Hs, Ws, th, tw):
                    served += rc == 0
                    refused += rc != 0
                    limited += rc == 0 and p[6] > LDS_AIM
    print("horizontal grid: %d plans, %d of them over 48 KB, %d refusals" % (served, limited, refused))
    assert served > 10000 and limited > 0 and refused > 0


def test_the_tap_tables_are_the_reference_restatement():
    """The float64 evaluation alone is tests/resized_crop_ref.py's (axis_weights' lo and hi), so the tables above check the formula
    the GPU tests compare against."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import resized_crop_ref as ref
    for n_in, n_out in ((5, 8), (64, 8), (40, 8), (256, 224), (9, 4), (520, 65), (1, 3)):
        lo, hi, _ = tap_tables(n_out)
        W = ref.axis_weights(n_in, n_out)
        for o in range(n_out):
            nz = np.nonzero(W[o].numpy())[0]
            assert lo[n_in - 1, o] <= nz[0] and nz[-1] < hi[n_in - 1, o]
        assert ref.taps(n_in, n_out) <= widest_support(n_out)[n_in - 1]


PINNED = [   # (Hs, Ws, th, tw), float (rpb, chunks), byte (rpb, chunks)
    ((256, 256, 224, 224), (16, 14), (15, 15)),
    ((80, 80, 64, 64), (64, 1), (59, 2)),
    ((512, 512, 64, 64), (1, 64), (1, 64)),
]


@pytest.mark.parametrize("geo,want_f,want_b", PINNED, ids=["%dx%d_to_%dx%d" % p[0] for p in PINNED])
def test_pinned_plans(geo, want_f, want_b):
    (rf, pf), (rb, pb) = check_geometry(*geo)
    assert rf == 0 and rb == 0 and pf[:2] == want_f and pb[:2] == want_b
    if geo == (512, 512, 64, 64):
        assert pb[6] == 49484 and pb[6] > LDS_AIM >= pf[6] and pf[6] == pb[6] - LUT_BYTES


def test_a_frame_whose_line_band_does_not_fit_is_refused():
    for byte in (False, True):
        assert plan(40, 1100, 5, 140, byte) == (ENOTSUP, (-99,) * 7)
        assert plan(1000, 1000, 125, 125, byte)[0] == ENOTSUP          # the header's example
    assert plan(560, 560, 70, 70, False)[0] == 0 and plan(560, 560, 70, 70, False)[1][6] > LDS_AIM


def test_argument_errors():
    from clsurvey_amd import _lib
    for args in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0), (-1, 8, 8, 8), (8, 8, 8, -5)):
        assert plan(*args, False) == (EINVAL, (-99,) * 7) and plan(*args, True)[0] == EINVAL
    assert _lib.lib().clhip_resized_crop_plan(8, 8, 8, 8, 0, None) == EINVAL


def test_crop_rows_per_block():
    """4096 output elements per block, one line from 4096 columns on; chunks of the crop geometries of the GPU tests."""
    from clsurvey_amd import _lib
    rows = _lib.lib().clhip_crop_rows_per_block
    for tw in list(range(1, 200)) + [1023, 1024, 1025, 2048, 2049, 4095]:
        assert rows(tw) == 4096 // tw
    for tw in (4096, 4097, 4100, 100000):
        assert rows(tw) == 1
    assert rows(0) == EINVAL and rows(-3) == EINVAL
    assert (rows(64), rows(63), rows(36), rows(224)) == (64, 65, 113, 18)
