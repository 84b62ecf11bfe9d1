"""Argument checks of the entry points of csrc/wino.hip (clhip_conv3x3_wino_fwd / _bwd_data / _bwd_weight / _bwd) and the workspace
sizes they report, against the launch rules restated in wino_dispatch.py.  Runs without a GPU: the pointers are dummies that are
never dereferenced, because every call here is turned down before it launches anything.

Order of the checks, read from the code:
  clhip_conv3x3_wino_fwd / _bwd_data   N <= 0 or a shape outside clhip_internal_wino_ok -> ENOTSUP;  a NULL x / w / y / ws (dy / w /
      dx / ws) or ws_bytes below clhip_internal_wino_ws -> EINVAL;  an odd map with arg-max codes -> ENOTSUP;  then the weight
      transform and the convolution launch.  Every accepted-shape call here has a short workspace or a NULL pointer, or is the
      odd-map-with-codes refusal.
  clhip_conv3x3_wino_bwd_weight        a NULL x / dy / dw / ws or N <= 0 -> EINVAL (N <= 0 is EINVAL here, not ENOTSUP);  a shape
      outside clhip_internal_wino_wgrad_ok, 2^29 or more elements of x or dy, or an odd map with codes -> ENOTSUP;  a workspace
      below one slab -> ENOSPC;  then the launch.  Every call here has a workspace below one slab.
  clhip_conv3x3_wino_bwd               a NULL x / dy / w / dx / dw / ws or N <= 0 -> EINVAL;  an odd map or a shape outside either
      domain -> ENOTSUP;  ws_bytes below clhip_conv3x3_wino_bwd_ws -> EINVAL;  a weight gradient that is not the 16-byte-staged
      pixel-split kernel, more than 256 pixels, a narrow map other than 8 x 8 -> ENOTSUP;  then the launches."""
import ctypes as C

import wino_dispatch as wd

EINVAL, ENOSPC, ENOTSUP = -1, -2, -3
BIG = 1 << 40


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(128)
    p = (C.addressof(buf) + 15) & ~15                   # 16-byte aligned: the weight gradient judges x | dy
    return L, p, buf


def test_case_table_follows_from_the_rules():
    wd.check_case_table()


def _shapes():
    grid = [(s[1], s[2], s[3], s[4]) for s, _ in wd.FWD_CASES] + list(wd.REFUSED)
    grid += [(Cc, K, H, W) for Cc in (16, 24, 64, 72, 128, 512) for K in (32, 64, 96, 160, 512) for H, W in ((8, 8), (4, 16), (13, 13), (5, 9), (12, 20), (7, 8), (9, 17))]
    return grid


def test_workspace_sizes_are_the_mirrors():
    L, p, _keep = _setup()
    for Cin, Cout, H, W in _shapes():
        assert L.clhip_conv3x3_wino_ws(Cin, Cout) == wd.conv3x3_wino_ws(Cin, Cout), (Cin, Cout)
    assert wd.wino_ws_bytes(24, 96) == 2 * 3 * 18432 * 4 and wd.wino_ws_bytes(16, 32) == 2 * 18432 * 4           # by hand
    shapes = [c[0] for c in wd.WG_CASES] + [s for s, _ in wd.PAIR_CASES] + [s[:5] for s in wd.PAIR_DECLINED]
    shapes += [(N, Cc, K, H, W) for N in (1, 7, 200) for Cc in (64, 128, 192, 1024) for K in (64, 256, 1024) for H, W in ((8, 8), (16, 16), (13, 13), (4, 8), (6, 18))]
    refused = [(2, 32, 64, 8, 8), (2, 64, 32, 8, 8), (2, 96, 64, 8, 8), (2, 64, 64, 3, 8), (2, 64, 64, 8, 7), (2, 64, 64, 2, 16),
               (0, 64, 64, 8, 8), (-1, 64, 64, 8, 8), (2, 0, 64, 8, 8), (2, 64, 0, 8, 8)]
    for s in shapes + refused:
        N, Cc, K, H, W = s
        want = wd.wgrad_ws_bytes(*s)
        assert (want == 0) == (s in refused or not wd.wgrad_ok(Cc, K, H, W)), s
        # the entry point reports the larger of the Winograd slabs and what the direct kernel (conv3x3_wgrad.hip) would ask for
        assert L.clhip_conv3x3_wino_bwd_weight_ws(*s) == max(want, L.clhip_conv3x3_bwd_weight_ws(*s)), s
        assert L.clhip_conv3x3_wino_bwd_ws(*s) == wd.wino_bwd_ws_bytes(*s), s
        assert (L.clhip_conv3x3_wino_bwd_ws(*s) == 0) == (want == 0), s
    # by hand: 64 -> 64 has one 64 x 64 tile -> 256 slabs of 9 * 64 * 64 + 64 floats; 1024 -> 1024 has 256 tiles -> one slab
    assert wd.wgrad_ws_bytes(2, 64, 64, 8, 8) == 256 * 36928 * 4 and wd.wgrad_ws_bytes(2, 1024, 1024, 8, 8) == (9 * 1024 * 1024 + 1024) * 4
    assert wd.wino_bwd_ws_bytes(3, 64, 64, 16, 16) == 8 * 18432 * 4 + 256 * 36928 * 4


def test_forward_and_backward_data_refusals():
    L, p, _keep = _setup()

    def fwd(ptrs, N, Cin, Cout, H, W, idx, ws, nbytes):
        x, w, b, y = ptrs
        return L.clhip_conv3x3_wino_fwd(x, w, b, y, idx, N, Cin, Cout, H, W, 1, ws, nbytes, None)

    def bwd(ptrs, N, Cin, Cout, H, W, idx, ws, nbytes):         # the kernel's (Cin, Cout) = the layer's (K, C)
        dy, w, src, dx = ptrs
        return L.clhip_conv3x3_wino_bwd_data(dy, idx, w, src, dx, N, Cout, Cin, H, W, ws, nbytes, None)

    for call in (fwd, bwd):
        for Cin, Cout, H, W in _shapes():
            ok = wd.wino_ok(Cin, Cout, H, W)
            need = wd.wino_ws_bytes(Cin, Cout)
            # outside the domain the shape is judged first: ENOTSUP whatever the pointers; inside, a workspace one byte short is EINVAL
            assert call([p, p, p, p], 2, Cin, Cout, H, W, None, p, need - 1) == (EINVAL if ok else ENOTSUP), (call.__name__, Cin, Cout, H, W)
            assert call([None, None, None, None], 2, Cin, Cout, H, W, None, None, 0) == (EINVAL if ok else ENOTSUP)
            for N in (0, -1):
                assert call([p, p, p, p], N, Cin, Cout, H, W, None, p, BIG) == ENOTSUP
            if not ok:
                assert call([p, p, p, p], 2, Cin, Cout, H, W, None, p, BIG) == ENOTSUP
                continue
            for null in (0, 1, 3):                               # the third pointer (bias / relu_src) is optional
                ptrs = [p, p, p, p]
                ptrs[null] = None
                assert call(ptrs, 2, Cin, Cout, H, W, None, p, BIG) == EINVAL
            assert call([p, p, p, p], 2, Cin, Cout, H, W, None, None, BIG) == EINVAL
            assert call([p, p, p, p], 2, Cin, Cout, H, W, None, p, 0) == EINVAL
            if (H | W) & 1:
                # arg-max codes on an odd map: refused BEFORE the weight transform (nothing is launched, so this runs without a GPU);
                # a short workspace is still EINVAL first
                assert call([p, p, p, p], 2, Cin, Cout, H, W, p, p, BIG) == ENOTSUP
                assert call([p, p, p, p], 2, Cin, Cout, H, W, p, p, need - 1) == EINVAL


def test_weight_gradient_refusals():
    L, p, _keep = _setup()

    def wg(ptrs, s, idx, ws, nbytes):
        x, dy, dw, db = ptrs
        return L.clhip_conv3x3_wino_bwd_weight(x, dy, idx, dw, db, *s, ws, nbytes, None)

    for case in wd.WG_CASES:
        s, pooled = case[0], case[1]
        N, Cc, K, H, W = s
        slab = wd.slab_floats(Cc, K) * 4
        for db in (p, None):                                     # db is optional
            assert wg([p, p, p, db], s, p if pooled else None, p, slab - 1) == ENOSPC, s
            assert wg([p, p, p, db], s, p if pooled else None, p, 0) == ENOSPC, s
        assert wd.wgrad_geo(*s, slab - 1) == ENOSPC
        for null in (0, 1, 2):
            ptrs = [p, p, p, p]
            ptrs[null] = None
            assert wg(ptrs, s, None, p, BIG) == EINVAL, s
        assert wg([p, p, p, p], s, None, None, BIG) == EINVAL, s
        for n in (0, -1):
            assert wg([p, p, p, p], (n,) + s[1:], None, p, BIG) == EINVAL, s
        if (H | W) & 1:                                          # odd maps with codes
            assert wd.wgrad_geo(*s, BIG, True, True) == ENOTSUP
            assert wg([p, p, p, p], s, p, p, BIG) == ENOTSUP, s
            assert wg([p, p, p, p], s, p, p, 0) == ENOTSUP, s   # ... judged before the workspace
    for s in ((2, 32, 64, 8, 8), (2, 64, 32, 8, 8), (2, 96, 64, 8, 8), (2, 64, 64, 3, 8), (2, 64, 64, 8, 7), (2, 64, 64, 2, 16), (2, 0, 64, 8, 8),
              (1 << 17, 64, 64, 8, 8), (1 << 15, 64, 256, 8, 8)):             # the last two: 2^29 elements of x and dy / of dy
        assert wd.wgrad_geo(*s, BIG) == ENOTSUP, s
        assert wg([p, p, p, p], s, None, p, BIG) == ENOTSUP, s
        assert wg([p, p, p, p], s, None, p, 0) == ENOTSUP, s
    s = ((1 << 17) - 1, 64, 64, 8, 8)                            # just under 2^29 elements: the shape passes, the workspace is judged
    assert wd.wgrad_geo(*s, 0) == ENOSPC and wg([p, p, p, p], s, None, p, 0) == ENOSPC


def test_one_grid_backward_refusals():
    L, p, _keep = _setup()

    def pair(ptrs, s, idx, ws, nbytes):
        x, dy, w, src, dx, dw, db = ptrs
        return L.clhip_conv3x3_wino_bwd(x, dy, idx, w, src, dx, dw, db, *s, ws, nbytes, None)

    full = [p] * 7
    for s6 in wd.PAIR_DECLINED:                                  # the shapes test_one_grid_backward_declines_other_shapes lists
        s, pooled = s6[:5], s6[5]
        assert not wd.pair_shape(*s6)
        assert pair(full, s, p if pooled else None, p, BIG) == ENOTSUP, s6
    # a layer whose weight gradient runs on the 64 x 64-tile kernel (512 blocks of one stage each would be 16 * splits > stages ... no:
    # 256 -> 256 has 16 tiles -> 16 splits, 200 stages < 256: pixel-split) — and one that does not: 1024 -> 1024, one slab, 200 >= 16
    assert wd.wgrad_geo(200, 1024, 1024, 8, 8, BIG) == wd.WgradGeo(False, False, True, 1, 256)
    assert pair(full, (200, 1024, 1024, 8, 8), None, p, BIG) == ENOTSUP
    for s, _plan in wd.PAIR_CASES:
        need = wd.wino_bwd_ws_bytes(*s)
        assert L.clhip_conv3x3_wino_bwd_ws(*s) == need > 0
        assert pair(full, s, None, p, need - 1) == EINVAL, s     # a short workspace is EINVAL here
        assert pair(full, s, None, p, 0) == EINVAL, s
        for null in (0, 1, 2, 4, 5):                             # relu_src (3) and db (6) are optional
            ptrs = list(full)
            ptrs[null] = None
            assert pair(ptrs, s, None, p, BIG) == EINVAL, (s, null)
        assert pair(full, s, None, None, BIG) == EINVAL
        for n in (0, -1):
            assert pair(full, (n,) + s[1:], None, p, BIG) == EINVAL
        # x or dy off a 16-byte boundary: the weight gradient would stage by scalars, which the merged grid does not hold
        assert wd.pair_plan(*s, aligned=False) is None
        assert pair([p + 4] + full[1:], s, None, p, BIG) == ENOTSUP and pair([p, p + 8] + full[2:], s, None, p, BIG) == ENOTSUP
