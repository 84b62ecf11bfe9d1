"""Argument checks of the five entry points of csrc/gem.hip (clhip_axpy, clhip_gem_gram, clhip_gem_project, clhip_gem_qp,
clhip_gem_project_dev) and the size clhip_gem_gram_ws reports.  Runs without a GPU: every call below is refused before
anything is launched, so the pointers are dummies that are never dereferenced (the row indices and the host coefficients,
which the entry points do read, are real arrays)."""
import ctypes as C

EINVAL = -1
GRAM_BLOCKS = 2048          # the block cap of the Gram pass: the workspace holds one partial per block and pair


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    return L, C.addressof(buf), buf


def _idx():
    return (C.c_int * 16)(*range(16))


def test_gram_ws_size():
    L, p, _keep = _setup()
    for m in range(1, 17):
        assert L.clhip_gem_gram_ws(m) == GRAM_BLOCKS * (m * (m + 1) // 2) * 8, m
    for m in (0, -1, 17, 18, 1 << 20, -(1 << 20)):
        assert L.clhip_gem_gram_ws(m) == 0, m


def test_axpy_rejects_null_pointers():
    L, p, _keep = _setup()
    for assign in (0, 1):
        assert L.clhip_axpy(None, p, 4, 1.0, assign, None) == EINVAL
        assert L.clhip_axpy(p, None, 4, 1.0, assign, None) == EINVAL
        assert L.clhip_axpy(None, None, 0, 1.0, assign, None) == EINVAL
        assert L.clhip_axpy(p, p, 0, 1.0, assign, None) == 0            # n = 0: nothing to do, nothing launched


def test_gram_rejects_bad_arguments():
    L, p, _keep = _setup()
    idx = _idx()
    big = L.clhip_gem_gram_ws(16)
    # (G, ld, row_idx, m, n, out, ws, ws_bytes, stream)
    good = [p, 8, idx, 3, 8, p, p, big, None]
    for null in (0, 2, 5, 6):
        a = list(good)
        a[null] = None
        assert L.clhip_gem_gram(*a) == EINVAL, null
    for m in (0, -1, 17, 1 << 20):
        a = list(good)
        a[3] = m
        assert L.clhip_gem_gram(*a) == EINVAL, m
    a = list(good)
    a[4] = 0
    assert L.clhip_gem_gram(*a) == EINVAL
    for m in range(1, 17):
        a = list(good)
        a[3], a[7] = m, L.clhip_gem_gram_ws(m) - 1
        assert L.clhip_gem_gram(*a) == EINVAL, m


def test_project_rejects_bad_arguments():
    L, p, _keep = _setup()
    idx = _idx()
    v = (C.c_float * 16)(*([0.5] * 16))
    # (G, ld, row_idx, v_host, m, g, out, n, stream)
    good = [p, 8, idx, v, 3, p, p, 8, None]
    for null in (0, 2, 3, 5, 6):
        a = list(good)
        a[null] = None
        assert L.clhip_gem_project(*a) == EINVAL, null
    for m in (0, -1, 17, 1 << 20):
        a = list(good)
        a[4] = m
        assert L.clhip_gem_project(*a) == EINVAL, m
    a = list(good)
    a[7] = 0
    assert L.clhip_gem_project(*a) == EINVAL


def test_project_dev_rejects_bad_arguments():
    L, p, _keep = _setup()
    idx = _idx()
    # (G, ld, row_idx, v_dev, info_dev, m, g, out, n, stream)
    good = [p, 8, idx, p, p, 3, p, p, 8, None]
    for null in (0, 2, 3, 4, 6, 7):
        a = list(good)
        a[null] = None
        assert L.clhip_gem_project_dev(*a) == EINVAL, null
    for m in (0, -1, 17, 1 << 20):
        a = list(good)
        a[5] = m
        assert L.clhip_gem_project_dev(*a) == EINVAL, m
    a = list(good)
    a[8] = 0
    assert L.clhip_gem_project_dev(*a) == EINVAL


def test_qp_rejects_bad_arguments():
    L, p, _keep = _setup()
    margin, eps = C.c_double(0.5), C.c_double(1e-3)
    # (gram, m, margin, eps, v_out, info, stream); m = memory rows + 1, so m = 2 is the smallest problem and 16 the largest
    for null in (0, 4, 5):
        a = [p, 3, margin, eps, p, p, None]
        a[null] = None
        assert L.clhip_gem_qp(*a) == EINVAL, null
    for m in (1, 0, -1, 17, 1 << 20):
        assert L.clhip_gem_qp(p, m, margin, eps, p, p, None) == EINVAL, m
