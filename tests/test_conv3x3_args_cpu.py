"""Argument checks of the entry points of csrc/conv3x3.hip and csrc/conv3x3_wgrad.hip (clhip_conv3x3_fwd / _relu_pool_fwd / _bwd_data /
_bwd_data_unpool / _bwd_weight_ws / _bwd_weight / _bwd_weight_unpool / _bwd_weight_slabs / _bwd_weight_reduce) and the workspace size
they report, against the launch rules restated in conv3x3_dispatch.py; and the odd-map refusal of clhip_conv3x3_bs_fwd / _bs_bwd_data.
Runs without a GPU: the pointers are dummies that are never dereferenced, because every call asserted on here is turned down
before it launches anything.  (A call that does reach a launch answers with a HIP error number on a machine without a GPU, never
with CLHIP_EINVAL: test_index_width_limits uses that to tell `refused` from `launched`.)

Order of the checks, read from the code:
  clhip_conv3x3_fwd / _bwd_data     a NULL x / w / y (dy / w / dx) or dimensions outside dims_ok -> EINVAL; then the launch.
  clhip_conv3x3_relu_pool_fwd       the same with y_pool and idx_u8, and an odd H or W -> EINVAL.
  clhip_conv3x3_bwd_data_unpool     NULL dy_pool / idx_u8 / w / dx or dims -> EINVAL; an odd map, a shape or pointer outside vec_ok, codes
                                    at an odd address -> ENOTSUP.
  clhip_conv3x3_bwd_weight*         NULL x / dy / dw / ws or dims -> EINVAL; codes on an odd map -> ENOTSUP; a workspace below
                                    clhip_conv3x3_bwd_weight_ws -> ENOSPC; the general kernel with codes off the 16-byte staging or at
                                    an odd address -> ENOTSUP; _unpool without codes, _slabs without splits_out or ws -> EINVAL first.
  clhip_conv3x3_bwd_weight_reduce   NULL ws / dw, K, C or splits <= 0 -> EINVAL.

Found with this file: the parent library took every positive dimension, so launch_geo multiplied tiles_w * tiles_h * ngrp past 2^31 in
int and the kernels formed byte offsets past 2^31 (test_index_width_limits on the parent: the calls reach the launch); and
clhip_conv3x3_bs_fwd / _bs_bwd_data answered an odd map with codes only after the weight launch (on the parent without a GPU: a HIP
error number instead of CLHIP_ENOTSUP)."""
import ctypes as C

import conv3x3_dispatch as d

EINVAL, ENOSPC, ENOTSUP = -1, -2, -3
BIG = 1 << 40
OK = (2, 8, 16, 8, 8)                                  # N, C, K, H, W


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(128)
    p = (C.addressof(buf) + 15) & ~15
    return L, p, buf


def test_error_codes_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "clhip.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define CLHIP_(E[A-Z]+) \((-\d+)\)", text)}
    assert got == {"EINVAL": EINVAL, "ENOSPC": ENOSPC, "ENOTSUP": ENOTSUP}


def test_case_tables_follow_from_the_rules():
    d.check_case_tables()


def test_workspace_size_is_make_plan():
    L, p, _keep = _setup()
    shapes = [c[0] for c in d.WG_CASES] + [s for s, _, _ in d.PS_SWITCH] + [d.CAP_CASE[0]] + [s for s, _ in d.FWD_CASES] + [s for s, _ in d.POOL_CASES]
    shapes += [(N, Cc, K, H, W) for N in (1, 7, 31, 32, 200) for Cc in (1, 3, 4, 24, 64, 65, 256, 960) for K in (1, 40, 64, 72, 512, 1024)
               for H, W in ((1, 1), (8, 8), (16, 16), (13, 13), (4, 8), (6, 18), (5, 9), (32, 32), (2, 64), (7, 35))]
    assert len(shapes) > 2000
    capped = 0
    for s in shapes:
        assert L.clhip_conv3x3_bwd_weight_ws(*s) == d.ws_bytes(*s) > 0, s
        p_ = d.make_plan(*s)
        capped += p_.splits < min(d.cdiv(1024 if s[1] * 9 <= 32 else 256, p_.k_tiles * p_.c_tiles), p_.total_stages)
    assert capped >= 1                                  # the 64 MB cap is reachable (conv3x3_dispatch's header): CAP_CASE and its like
    for i in range(5):
        for v in (0, -1):
            s = list(OK)
            s[i] = v
            assert L.clhip_conv3x3_bwd_weight_ws(*s) == 0, s
    # by hand: (2, 64, 64, 8, 8): 2 stages < 8 -> pixel-split, 4 tiles of 32 x 32, splits = min(64, 2) = 2, groups of 2: 1 -> 3 slabs of 36928
    assert d.ws_bytes(2, 64, 64, 8, 8) == 3 * 36928 * 4


def _entries(L, p):
    """name -> call(ptrs, shape, idx, ws, ws_bytes): ptrs are the four float pointers of the entry in its own order."""
    so = C.c_int(0)

    def fwd(q, s, idx, ws, n):
        return L.clhip_conv3x3_fwd(q[0], q[1], q[2], q[3], *s, 1, None)

    def pool(q, s, idx, ws, n):
        return L.clhip_conv3x3_relu_pool_fwd(q[0], q[1], q[2], q[3], idx, *s, None)

    def bwd(q, s, idx, ws, n):
        return L.clhip_conv3x3_bwd_data(q[0], q[1], q[2], q[3], *s, None)

    def bwd_u(q, s, idx, ws, n):
        return L.clhip_conv3x3_bwd_data_unpool(q[0], idx, q[1], q[2], q[3], *s, None)

    def wg(q, s, idx, ws, n):
        return L.clhip_conv3x3_bwd_weight(q[0], q[1], q[2], q[3], *s, ws, n, None)

    def wg_u(q, s, idx, ws, n):
        return L.clhip_conv3x3_bwd_weight_unpool(q[0], q[1], idx, q[2], q[3], *s, ws, n, None)

    def slabs(q, s, idx, ws, n):
        return L.clhip_conv3x3_bwd_weight_slabs(q[0], q[1], idx, *s, ws, n, C.byref(so), None)
    return dict(fwd=fwd, pool=pool, bwd=bwd, bwd_u=bwd_u, wg=wg, wg_u=wg_u, slabs=slabs)


def test_null_pointers_and_non_positive_dimensions():
    L, p, _keep = _setup()
    E = _entries(L, p)
    full = [p, p, p, p]
    required = dict(fwd=(0, 1, 3), pool=(0, 1, 3), bwd=(0, 1, 3), bwd_u=(0, 1, 3), wg=(0, 1, 2), wg_u=(0, 1, 2), slabs=(0, 1))
    for name, call in E.items():
        for null in required[name]:
            q = list(full)
            q[null] = None
            assert call(q, OK, p, p, BIG) == EINVAL, (name, null)
        for i in range(5):
            for v in (0, -1):
                s = list(OK)
                s[i] = v
                assert call(full, s, p, p, BIG) == EINVAL, (name, s)
    for name in ("wg", "wg_u", "slabs"):
        assert E[name](full, OK, p, None, BIG) == EINVAL, name              # ws is required
    assert E["pool"](full, OK, None, p, BIG) == EINVAL and E["bwd_u"](full, OK, None, p, BIG) == EINVAL      # the codes
    assert E["wg_u"](full, OK, None, p, BIG) == EINVAL                      # bwd_weight_unpool without codes
    assert L.clhip_conv3x3_bwd_weight_slabs(p, p, None, *OK, p, BIG, None, None) == EINVAL      # without splits_out
    for odd in ((2, 8, 16, 7, 8), (2, 8, 16, 8, 7), (2, 3, 16, 7, 32), (2, 3, 16, 8, 33)):
        assert E["pool"](full, odd, p, p, BIG) == EINVAL, odd                # relu_pool_fwd on an odd map
    # _reduce
    assert L.clhip_conv3x3_bwd_weight_reduce(None, p, p, 16, 8, 4, None) == EINVAL and L.clhip_conv3x3_bwd_weight_reduce(p, None, p, 16, 8, 4, None) == EINVAL
    for K, Cc, splits in ((0, 8, 4), (16, 0, 4), (16, 8, 0), (16, 8, -1), (-1, 8, 4)):
        assert L.clhip_conv3x3_bwd_weight_reduce(p, p, p, K, Cc, splits, None) == EINVAL, (K, Cc, splits)


def test_unpool_refusals():
    L, p, _keep = _setup()
    E = _entries(L, p)
    full = [p, p, p, p]
    # backward-data from pooled dy: odd maps, shapes outside vec_ok (K % 8, C % 4, W % 4, W % TW), misaligned dy | w, odd code address
    for s in ((2, 8, 16, 7, 8), (2, 8, 16, 8, 9), (2, 8, 12, 8, 8), (2, 6, 16, 8, 8), (2, 8, 16, 8, 6), (2, 8, 16, 8, 12), (2, 8, 16, 8, 24), (2, 8, 16, 4, 40)):
        assert d.bwd_plan(*s, unpool=True) == ENOTSUP, s
        assert E["bwd_u"](full, s, p, p, BIG) == ENOTSUP, s
    assert d.bwd_plan(*OK, unpool=True) != ENOTSUP and d.bwd_plan(*OK, aligned=False, unpool=True) == ENOTSUP
    assert E["bwd_u"]([p + 4, p, p, p], OK, p, p, BIG) == ENOTSUP and E["bwd_u"]([p, p + 8, p, p], OK, p, p, BIG) == ENOTSUP
    assert E["bwd_u"](full, OK, p + 1, p, BIG) == ENOTSUP and E["bwd_u"](full, OK, p + 3, p, BIG) == ENOTSUP
    # the weight gradient with codes: odd maps are judged before the workspace, the rest behind it
    for s, al in d.WG_REFUSED:
        q = [p + (0 if al[0] else 4), p + (0 if al[1] else 8), p, p]
        idx = p + (1 if al[2] == 1 else 0)
        need = d.ws_bytes(*s)
        for name in ("wg_u", "slabs"):
            assert E[name](q, s, idx, p, BIG) == ENOTSUP, (name, s, al)
            assert E[name](q, s, idx, p, need - 1) == (ENOTSUP if (s[3] | s[4]) & 1 else ENOSPC), (name, s, al)


def test_short_workspace():
    L, p, _keep = _setup()
    E = _entries(L, p)
    full = [p, p, p, p]
    for case in d.WG_CASES + [(d.CAP_CASE[0], False, d.AL, None, None)] + [(s, False, d.AL, None, None) for s, _, _ in d.PS_SWITCH]:
        s, pooled = case[0], case[1]
        need = L.clhip_conv3x3_bwd_weight_ws(*s)
        for nbytes in (need - 1, 0):
            assert E["wg_u" if pooled else "wg"](full, s, p, p, nbytes) == ENOSPC, s
            assert E["slabs"](full, s, p if pooled else None, p, nbytes) == ENOSPC, s


def test_index_width_limits():
    """Dimensions whose tile counts or per-image byte offsets pass 2^31 in the kernels' int arithmetic (conv3x3_dispatch.dims_ok):
    CLHIP_EINVAL from every entry point before any launch, and a workspace size of 0; just inside each limit the shape passes (the weight
    gradient goes on to its workspace check, forward and backward-data to the launch, which is anything but EINVAL)."""
    L, p, _keep = _setup()
    E = _entries(L, p)
    full = [p, p, p, p]
    M = 0x7fffffff
    beyond = [(M, 8, 8, 64, 64), (M, M, M, M, M), (1 << 20, 8, 8, 64, 32),           # N H W > 2^31 - 1: launch_geo's int tile count
              (1, 8, 8, 4096, 2048), (1, 1, 1, 1 << 12, 1 << 11),                     # H W = 2^23
              (1, 8, 8, 2048, 3277), (1, 1, 1, 1 << 12, 1986),                        # 40 H W = 268 451 840, 33 H W = 268 443 648 >= 2^28
              (1, 1 << 14, 8, 128, 128), (1, 8, 1 << 14, 128, 128),                   # C H W = 2^28, K H W = 2^28
              (1, (1 << 14) - 32, 8, 128, 128), (1, 8, (1 << 14) - 32, 128, 128),     # (C + 32) H W = 2^28, (K + 32) H W = 2^28
              (1, 1 << 13, 7282, 2, 2), (1, 65536, 65536, 1, 1)]                      # 9 K C >= 2^29
    for s in beyond:
        assert not d.dims_ok(*s), s
        assert L.clhip_conv3x3_bwd_weight_ws(*s) == 0, s
        for name, call in E.items():
            if name in ("pool", "bwd_u", "wg_u") and (s[3] | s[4]) & 1:
                continue
            assert call(full, s, p, p, BIG) == EINVAL, (name, s)
    inside = [((1 << 19) - 1, 8, 8, 64, 64), (1, 8, 8, 2048, 3276), (1, 1, 1, 1 << 12, 1985),           # 40 H W = 268 369 920, 33 H W = 268 308 480
              (1, (1 << 14) - 33, 8, 128, 128), (1, 8, (1 << 14) - 33, 128, 128), (1, 1 << 13, 7281, 2, 2)]
    for s in inside:
        assert d.dims_ok(*s), s
        assert L.clhip_conv3x3_bwd_weight_ws(*s) == d.ws_bytes(*s) > 0, s
        assert E["wg"](full, s, None, p, 0) == ENOSPC and E["slabs"](full, s, None, p, 0) == ENOSPC, s
    # accepted calls do not change: a small shape goes through to the launch (no GPU here: a HIP error number; with one: 0 is not asked)
    import torch
    if not torch.cuda.is_available():
        x = (C.c_float * 4096)()
        q = [C.addressof(x)] * 4
        for name in ("fwd", "bwd"):
            assert E[name](q, (1, 8, 8, 4, 8), None, None, 0) not in (EINVAL, ENOSPC, ENOTSUP), name


def test_bs_entries_refuse_codes_on_an_odd_map_before_the_weight_launch():
    """clhip_conv3x3_bs_fwd / _bs_bwd_data pass clhip_internal_bs_ok on an odd map; with arg-max codes they must answer CLHIP_ENOTSUP
    before clhip_internal_bs_weights is launched into the workspace — so without a GPU the answer is ENOTSUP and no HIP error."""
    L, p, _keep = _setup()
    for H, W in ((5, 9), (8, 9), (5, 8)):
        need = L.clhip_conv3x3_bs_ws(64, 64)
        assert need > 0
        assert L.clhip_conv3x3_bs_fwd(p, p, p, p, p, 2, 64, 64, H, W, 1, p, need, None) == ENOTSUP
        assert L.clhip_conv3x3_bs_bwd_data(p, p, p, p, p, 2, 64, 64, H, W, p, need, None) == ENOTSUP
        # the earlier checks keep their order: a short workspace or a NULL pointer is EINVAL first
        assert L.clhip_conv3x3_bs_fwd(p, p, p, p, p, 2, 64, 64, H, W, 1, p, need - 1, None) == EINVAL
        assert L.clhip_conv3x3_bs_bwd_data(None, p, p, p, p, 2, 64, 64, H, W, p, need, None) == EINVAL
