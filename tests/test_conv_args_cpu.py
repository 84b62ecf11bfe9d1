"""Argument checks of the entry points of csrc/conv2d.hip, the 5x5 entry points of csrc/bsconv.hip and csrc/bswgrad5.hip, and the
workspace sizes they report, against the launch rules restated in conv_dispatch.py.  Runs without a GPU: the pointers are dummies
that are never dereferenced, because every call here is turned down before it launches anything."""
import ctypes as C

import conv_dispatch as cd

EINVAL, ENOSPC, ENOTSUP = -1, -2, -3
OK_SHAPE = (2, 3, 8, 8, 4, 3, 3, 1, 1)           # N, C, H, W, K, R, S, stride, pad


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    return L, C.addressof(buf), buf


def _three(L, p, shape, ptrs_f=None, ptrs_d=None, ptrs_w=None, ws=None, ws_bytes=0):
    """The three clhip_conv2d_* calls on one shape; bwd_weight gets a workspace of 0 bytes unless told otherwise, so a shape that
    passes its checks answers ENOSPC instead of launching."""
    f = ptrs_f or [p, p, p, p]
    d = ptrs_d or [p, p, p, p]
    w = ptrs_w or [p, p, p, p]
    return (L.clhip_conv2d_fwd(*f, *shape, 1, None), L.clhip_conv2d_bwd_data(*d, *shape, None),
            L.clhip_conv2d_bwd_weight(*w, *shape, p if ws is None else ws, ws_bytes, None))


def test_conv2d_entries_reject_bad_arguments():
    L, p, _keep = _setup()
    assert cd.conv_ok(*OK_SHAPE) is not None and L.clhip_conv2d_bwd_weight_ws(*OK_SHAPE) > 0
    # (x, w, b, y), (dy, w, relu_src, dx): the third is optional; (x, dy, dw, db): db is optional, ws is required
    for null in (0, 1, 3):
        ptrs = [p, p, p, p]
        ptrs[null] = None
        assert L.clhip_conv2d_fwd(*ptrs, *OK_SHAPE, 1, None) == EINVAL
        assert L.clhip_conv2d_bwd_data(*ptrs, *OK_SHAPE, None) == EINVAL
    for null in (0, 1, 2):
        ptrs = [p, p, p, p]
        ptrs[null] = None
        assert L.clhip_conv2d_bwd_weight(*ptrs, *OK_SHAPE, p, 1 << 30, None) == EINVAL
    assert L.clhip_conv2d_bwd_weight(p, p, p, p, *OK_SHAPE, None, 1 << 30, None) == EINVAL
    bad = []
    for i in range(8):                                     # every dimension and the stride: 0 and negative
        for v in (0, -1):
            s = list(OK_SHAPE)
            s[i] = v
            bad.append(tuple(s))
    bad.append(OK_SHAPE[:8] + (-1,))                       # negative padding
    bad += [(1, 1, 300, 300, 1, 256, 3, 1, 0), (1, 1, 300, 300, 1, 3, 256, 1, 0)]                  # R or S above 255
    bad += [(1, 1, 2, 8, 1, 3, 3, 1, 0), (1, 1, 8, 2, 1, 3, 3, 1, 0)]                              # window larger than the padded map
    bad += [(1, 1, 1, 8, 1, 4, 3, 4, 0), (1, 1, 8, 1, 1, 3, 4, 4, 0)]                              # ... with a stride above the deficit
    bad += [(1, 1, 23171, 23171, 1, 3, 3, 23171, 0)]                                              # N*C*H*W = 23171^2 > 0x1fffffff
    bad += [(1, 1, 4096, 4096, 33, 1, 1, 1, 0)]                                                    # N*K*OH*OW = 33 * 2^24 > 0x1fffffff
    assert 1 * 1 * 23171 * 23171 > cd.MAX_ELEMS and 4096 * 4096 <= cd.MAX_ELEMS < 33 * 4096 * 4096
    for s in bad:
        assert cd.conv_ok(*s) is None, s
        assert _three(L, p, s, ws_bytes=1 << 40) == (EINVAL, EINVAL, EINVAL), s
        assert L.clhip_conv2d_bwd_weight_ws(*s) == 0, s
    # just inside the two element limits nothing is refused for size: bwd_weight reaches its workspace check
    for s in ((1, 1, 23170, 23170, 1, 3, 3, 23170, 0), (1, 1, 4096, 4096, 31, 1, 1, 1, 0)):
        assert cd.conv_ok(*s) is not None
        assert L.clhip_conv2d_bwd_weight_ws(*s) == cd.bwd_weight_ws_bytes(s) > 0
        assert L.clhip_conv2d_bwd_weight(p, p, p, p, *s, p, 0, None) == ENOSPC


def test_conv2d_tap_table_limit():
    """Forward and backward-data keep a table of R*S <= 256 taps in LDS: CLHIP_ENOTSUP above.  The weight gradient has no such
    table and takes the shape: it reports a workspace and goes on to its workspace check."""
    L, p, _keep = _setup()
    for s in ((1, 2, 20, 20, 3, 17, 16, 1, 0), (1, 2, 20, 20, 3, 16, 17, 1, 2), (1, 1, 255, 255, 1, 255, 255, 1, 0)):
        assert s[5] * s[6] > cd.TAB_MAX and cd.conv_ok(*s) is not None
        need = L.clhip_conv2d_bwd_weight_ws(*s)
        assert need == cd.bwd_weight_ws_bytes(s) > 0
        assert _three(L, p, s, ws_bytes=need - 1) == (ENOTSUP, ENOTSUP, ENOSPC), s
    s = (1, 2, 20, 20, 3, 16, 16, 1, 0)                    # exactly 256 taps: taken (nothing to observe without a GPU but the size)
    assert L.clhip_conv2d_bwd_weight_ws(*s) == cd.bwd_weight_ws_bytes(s) > 0


def test_conv2d_bwd_weight_ws_is_the_mirrors():
    L, p, _keep = _setup()
    cd.check_case_table()                                   # the hand-worked rows follow from the restated rules; all 17 instantiations
    grid = [s for s, _, _ in cd.CASES]
    grid += [(128, 3, 224, 224, 64, 11, 11, 4, 2), (128, 64, 27, 27, 192, 5, 5, 1, 2), (128, 192, 13, 13, 384, 3, 3, 1, 1),
             (128, 384, 13, 13, 256, 3, 3, 1, 1), (128, 256, 13, 13, 256, 3, 3, 1, 1)]              # AlexNet's layers
    grid += [(N, Cc, 9, 10, K, R, R, st, 1) for N in (1, 7, 64) for Cc in (1, 8, 65) for K in (1, 64, 65, 129, 200) for R in (1, 3) for st in (1, 2)]
    assert len(set(grid)) >= 190
    for s in grid:
        N, Cc, H, W, K, R, S, st, pad = s
        M, Nn, Kd = cd.gemm_dims("bwd_weight", s)
        splits = cd.wgrad_splits(M, Nn, Kd)
        slabs, bias = 4 * K * Cc * R * S * splits, 8 * K * cd.BIAS_SPLIT
        got = L.clhip_conv2d_bwd_weight_ws(*s)
        assert got == max(slabs, bias) == cd.bwd_weight_ws_bytes(s), (s, got, slabs, bias)
        # one byte short: without db only the slabs count, with db the bias partials as well
        assert L.clhip_conv2d_bwd_weight(p, p, p, None, *s, p, slabs - 1, None) == ENOSPC, s
        assert L.clhip_conv2d_bwd_weight(p, p, p, p, *s, p, got - 1, None) == ENOSPC, s
        assert L.clhip_conv2d_bwd_weight(p, p, p, p, *s, p, 0, None) == ENOSPC, s


def test_conv5x5_bs_sizes_and_refusals():
    L, p, _keep = _setup()
    cd.check_bs_tables()
    for Cc in (0, 16, 32, 33, 64, 96, 192):
        for K in (0, 32, 64, 65, 96, 192):
            assert L.clhip_conv5x5_bs_ws(Cc, K) == cd.bs5_ws_bytes(Cc, K), (Cc, K)
    big = 1 << 40
    shapes = [s for s, _, _, _ in cd.BS5_CASES]
    # just outside each condition of the domain: channels, H, W (W = 8 is inside clhip_internal_bs_ok but not the 5x5 entry points), N
    shapes += [(1, 16, 64, 4, 9), (1, 48, 64, 4, 9), (1, 32, 32, 4, 9), (1, 64, 96, 4, 9), (1, 64, 64, 3, 9), (1, 64, 64, 4, 8),
               (0, 64, 64, 4, 9), (-1, 64, 64, 4, 9), (1, 64, 64, 4, 9), (1, 64, 64, 4, 16), (1, 64, 64, 4, 17)]
    for N, Cc, K, H, W in shapes:
        okf, okd = cd.bs5_ok("fwd", N, Cc, K, H, W), cd.bs5_ok("bwd_data", N, Cc, K, H, W)
        rf = L.clhip_conv5x5_bs_fwd(p, p, p, p, N, Cc, K, H, W, 1, p, 0, None)            # a workspace of 0 bytes: nothing launches
        rd = L.clhip_conv5x5_bs_bwd_data(p, p, p, p, N, Cc, K, H, W, p, 0, None)
        assert rf == (EINVAL if okf else ENOTSUP), ((N, Cc, K, H, W), rf)
        assert rd == (EINVAL if okd else ENOTSUP), ((N, Cc, K, H, W), rd)
        if okf:
            need = cd.bs5_image_bytes(Cc, K)
            assert 0 < need <= L.clhip_conv5x5_bs_ws(Cc, K)
            assert L.clhip_conv5x5_bs_fwd(p, p, p, p, N, Cc, K, H, W, 1, p, need - 1, None) == EINVAL     # a short workspace is EINVAL here
            for null in (0, 1, 3):
                ptrs = [p, p, p, p]
                ptrs[null] = None
                assert L.clhip_conv5x5_bs_fwd(*ptrs, N, Cc, K, H, W, 1, p, big, None) == EINVAL
            assert L.clhip_conv5x5_bs_fwd(p, p, p, p, N, Cc, K, H, W, 1, None, big, None) == EINVAL
        if okd:
            need = cd.bs5_image_bytes(K, Cc)
            assert L.clhip_conv5x5_bs_bwd_data(p, p, p, p, N, Cc, K, H, W, p, need - 1, None) == EINVAL
            for null in (0, 1, 3):
                ptrs = [p, p, p, p]
                ptrs[null] = None
                assert L.clhip_conv5x5_bs_bwd_data(*ptrs, N, Cc, K, H, W, p, big, None) == EINVAL
            assert L.clhip_conv5x5_bs_bwd_data(p, p, p, p, N, Cc, K, H, W, None, big, None) == EINVAL


def test_conv5x5_bs_bwd_weight_sizes_and_refusals():
    L, p, _keep = _setup()
    big = 1 << 40
    shapes = [s for s, _, _ in cd.BSK5_CASES] + [(128, 64, 192, 27, 27)]
    shapes += [(1, 32, 32, 1, 7), (1, 16, 32, 1, 8), (1, 48, 32, 1, 8), (1, 32, 16, 1, 8), (1, 32, 48, 1, 8), (0, 32, 32, 1, 8),
               (1, 32, 32, 0, 8), (1, 0, 32, 1, 8), (1, 32, 0, 1, 8), (1, 32, 32, 1, 9), (1, 32, 32, 1, 16), (1, 32, 32, 1, 17),
               (4096, 32, 32, 64, 64), (4095, 32, 32, 64, 64)]                                    # 2^31 bytes of x: outside; just under: inside
    assert not cd.bsk5_ok(4096, 32, 32, 64, 64) and cd.bsk5_ok(4095, 32, 32, 64, 64)
    for s in shapes:
        ok = cd.bsk5_ok(*s)
        need = L.clhip_conv5x5_bs_bwd_weight_ws(*s)
        assert need == cd.bsk5_ws_bytes(*s) and (need > 0) == ok, (s, need)
        if not ok:
            assert L.clhip_conv5x5_bs_bwd_weight(p, p, p, p, *s, p, big, None) == ENOTSUP, s
            assert L.clhip_conv5x5_bs_bwd_weight(None, None, None, None, *s, None, 0, None) == ENOTSUP, s      # the shape is judged first
            continue
        for null in (0, 1, 2):
            ptrs = [p, p, p, p]
            ptrs[null] = None
            assert L.clhip_conv5x5_bs_bwd_weight(*ptrs, *s, p, big, None) == EINVAL, s
        assert L.clhip_conv5x5_bs_bwd_weight(p, p, p, p, *s, None, big, None) == EINVAL, s
        for db in (p, None):
            assert L.clhip_conv5x5_bs_bwd_weight(p, p, p, db, *s, p, need - 1, None) == ENOSPC, s
