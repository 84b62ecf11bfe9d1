"""Argument checks of the entry points of csrc/gemm.hip and the size clhip_fc_ws reports, against the launch rules restated
in gemm_dispatch.py.  Runs without a GPU: the pointers are dummies that are never dereferenced, because nothing is launched."""
import ctypes as C

import gemm_dispatch as gd

EINVAL = -1


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    return L, C.addressof(buf), buf


def test_fc_entries_reject_bad_arguments():
    L, p, _keep = _setup()
    bad_dims = [(0, 8, 5), (4, 0, 5), (4, 8, 0), (-1, 8, 5), (4, -2, 5), (4, 8, -3)]
    # (x, w, b, y), (dy, w, relu_src, dx), (x, dy, dw, db): the third of forward / backward-data and db are optional
    for null in (0, 1, 3):
        ptrs = [p, p, p, p]
        ptrs[null] = None
        assert L.clhip_fc_fwd(*ptrs, 4, 8, 5, 1, p, 64, None) == EINVAL
        assert L.clhip_fc_bwd_data(*ptrs, 4, 8, 5, p, 64, None) == EINVAL
    for null in (0, 1, 2):
        ptrs = [p, p, p, p]
        ptrs[null] = None
        assert L.clhip_fc_bwd_weight(*ptrs, 4, 8, 5, p, 64, None) == EINVAL
    for M, I, O in bad_dims:
        assert L.clhip_fc_fwd(p, p, p, p, M, I, O, 1, p, 64, None) == EINVAL
        assert L.clhip_fc_bwd_data(p, p, p, p, M, I, O, p, 64, None) == EINVAL
        assert L.clhip_fc_bwd_weight(p, p, p, p, M, I, O, p, 64, None) == EINVAL


def test_fc_ws_covers_its_three_calls():
    L, p, _keep = _setup()
    gd.check_case_table()                                   # the hand-worked rows of CASES follow from the restated rules
    for M, I, O in ((0, 8, 5), (4, 0, 5), (4, 8, 0), (-1, 8, 5), (4, -1, 5), (4, 8, -1), (0, 0, 0)):
        assert L.clhip_fc_ws(M, I, O) == 0 and gd.fc_ws_bytes(M, I, O) == 0
    grid = [s for s, _ in gd.CASES]
    grid += [(200, 2048, 128), (200, 128, 128), (200, 128, 20), (128, 9216, 4096), (128, 4096, 4096)]      # the product's layers
    grid += [(M, I, O) for M in (1, 63, 64, 65, 128, 200, 512) for I in (1, 95, 96, 128, 1024, 3104) for O in (5, 64, 127, 1024, 1028)]
    assert len(set(grid)) >= 200
    for M, I, O in grid:
        needs = [gd.fc_plan(kind, M, I, O).need_bytes for kind in gd.KINDS]
        twins = [gd.fc_plan(kind, M, I, O, a_aligned=False).need_bytes for kind in gd.KINDS]         # the same call declined to 64x64 tiles
        got = L.clhip_fc_ws(M, I, O)
        assert got == gd.fc_ws_bytes(M, I, O), (M, I, O, got)
        assert got >= max(needs + twins), (M, I, O, got, needs, twins)
        # clhip_fc_ws counts one slab for a call that runs unsplit (and then needs no workspace at all), so it exceeds the
        # largest per-call need exactly when its largest term belongs to an unsplit call
        terms = []
        for kind in gd.KINDS:
            g = gd.fc_gemm(kind, M, I, O)
            terms += [(4 * g.M * g.N * s, s) for s in (gd.choose_splits(g.M, g.N, g.K), gd.choose_splits_wide(g.M, g.N, g.K))]
        assert got == max(terms)[0]
        assert got == max(needs + twins) or all(s == 1 for nbytes, s in terms if nbytes == got), (M, I, O, got, needs, twins)
