"""Wide herding (clhip_icarl_herd_wide, F <= 16384) without a GPU: the exported symbols, the workspace size, every refusal of the
entry with dummy pointers (each call fails its checks before anything is dereferenced or launched), the wrapper's limit."""
import ctypes as C

import pytest

WIDE = 16384                                          # CLHIP_ICARL_MAX_FEATS_WIDE (include/clhip.h)


def _lib_and_table():
    from clsurvey_amd import _lib
    L = _lib.lib()
    tab = (_lib.IcarlClass * 2)()
    tab[0].row_begin, tab[0].row_end, tab[0].k, tab[0].out_off = 0, 3, 2, 0
    tab[1].row_begin, tab[1].row_end, tab[1].k, tab[1].out_off = 3, 4, 1, 2
    return L, tab


def test_both_symbols_are_exported_with_signatures():
    from clsurvey_amd import _lib
    L = _lib.lib()
    for name in ("clhip_icarl_herd_wide", "clhip_icarl_herd_wide_ws"):
        assert name in _lib.SIGNATURES and callable(getattr(L, name))
    assert L.clhip_icarl_herd_wide_ws.restype is C.c_size_t
    assert len(_lib.SIGNATURES["clhip_icarl_herd_wide"][1]) == len(_lib.SIGNATURES["clhip_icarl_herd"][1]) + 2


def test_workspace_is_two_fp32_vectors_per_class():
    """n_classes * 2 * F * 4 bytes exactly (the header documents: no rounding); 0 for an n_classes or F outside the limits, so a
    caller that sizes its buffer with it is refused by the entry and not by an overflow."""
    L, _ = _lib_and_table()
    for n, F in ((1, 1), (1, 4097), (4, 8192), (20, 16384), (128, 16384), (3, 260)):
        assert L.clhip_icarl_herd_wide_ws(n, F) == n * 2 * F * 4, (n, F)
    for n, F in ((0, 8), (129, 8), (-1, 8), (1, 0), (1, -4), (1, WIDE + 1)):
        assert L.clhip_icarl_herd_wide_ws(n, F) == 0, (n, F)


def test_wide_entry_rejects_bad_arguments():
    """Everything clhip_icarl_herd checks (tests/test_icarl_cpu.py), then F above 16384, a NULL workspace and one a byte short: -1
    (CLHIP_EINVAL) every time, before any launch."""
    L, tab = _lib_and_table()
    buf = C.create_string_buffer(64)                  # (never dereferenced: every call below fails its checks first)
    p = C.addressof(buf)
    F = 8
    need = L.clhip_icarl_herd_wide_ws(2, F)
    assert need == 2 * 2 * F * 4

    def call(feats=p, n_rows=4, F=F, w=p, table=tab, n_classes=2, ranking=p, ranking_len=3, ws=p, ws_bytes=need):
        return L.clhip_icarl_herd_wide(feats, n_rows, F, w, table, n_classes, ranking, ranking_len, ws, ws_bytes, None)

    assert call(feats=None) == -1 and call(w=None) == -1 and call(table=None) == -1 and call(ranking=None) == -1
    assert call(n_rows=0) == -1 and call(F=0) == -1 and call(F=-8) == -1
    assert call(n_classes=0) == -1 and call(n_classes=129) == -1
    assert call(n_rows=3) == -1                       # rows outside feats
    assert call(ranking_len=2) == -1                  # ranking too short
    tab[0].k = 4
    assert call(ranking_len=8) == -1                  # more picks than rows
    tab[0].k, tab[0].out_off = 2, -1
    assert call() == -1
    tab[0].out_off, tab[0].row_begin = 0, -1
    assert call() == -1
    tab[0].row_begin, tab[1].row_end = 0, 3
    assert call() == -1                               # an empty class
    tab[1].row_end = 3 + 65537
    assert call(n_rows=1 << 20) == -1                 # more rows in a class than CLHIP_ICARL_MAX_CLASS_ROWS
    tab[1].row_end = 4
    # the table is good again: only the width and the workspace are left to refuse
    assert call(F=WIDE + 1, ws_bytes=1 << 40) == -1
    assert call(F=1 << 30, ws_bytes=1 << 40) == -1
    assert call(ws=None) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    big = L.clhip_icarl_herd_wide_ws(2, WIDE)
    assert call(F=WIDE, ws_bytes=big - 1) == -1


def test_16384_features_pass_the_size_function_the_entry_checks_with():
    """F = 16384 with enough workspace is refused by nothing before the launch, and the launch is not made without a device.  What
    can be asserted here: the size function, whose value the entry compares ws_bytes against, takes 16384 and not 16385; and at
    16384 the one-byte-short workspace is what the entry refuses (above), so the width check before it let 16384 through."""
    L, _ = _lib_and_table()
    assert L.clhip_icarl_herd_wide_ws(2, WIDE) == 2 * 2 * WIDE * 4 > 0
    assert L.clhip_icarl_herd_wide_ws(2, WIDE + 1) == 0
    # the narrow entry and its limit stay
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    _, tab = _lib_and_table()
    assert L.clhip_icarl_herd(p, 4, 4097, p, tab, 2, p, 3, None) == -1


def test_wrapper_limit_is_the_wide_kernel_s():
    from clsurvey_amd import ops
    from clsurvey_amd.methods import icarl
    assert icarl.HERD_MAX_FEATS == 16384 == WIDE
    assert ops.ICARL_MAX_FEATS == 4096


def test_ops_refuses_host_tensors_on_either_entry():
    import torch
    from clsurvey_amd import ops
    f, w = torch.zeros(4, 8), torch.zeros(4)
    for wide in (None, True, False):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.icarl_herd(f, w, [(0, 4)], [1], wide=wide)
