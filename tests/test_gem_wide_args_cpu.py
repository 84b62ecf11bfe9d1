"""Argument checks of the entry points of csrc/gem_wide.hip (clhip_gem_gram_wide, clhip_gem_qp_wide, clhip_gem_project_wide,
clhip_gem_project_dev_wide) and the sizes clhip_gem_gram_wide_ws / clhip_gem_qp_wide_ws report.  Runs without a GPU: every call
below is refused before anything is launched, so the pointers are dummies that are never dereferenced (the row indices and the
host coefficients, which the entry points do read, are real arrays)."""
import ctypes as C

EINVAL = -1
WIDE_MAX = 64               # CLHIP_GEM_WIDE_MAX: rows of a Gram matrix
GRAM_WIDE_BLOCKS = 1024     # the block cap of the wide Gram pass: the workspace holds one 16 x 16 f64 tile per block and panel pair


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    return L, C.addressof(buf), buf


def _idx():
    return (C.c_int * WIDE_MAX)(*range(WIDE_MAX))


def _pairs(m):
    panels = (m + 15) // 16
    return panels * (panels + 1) // 2


def test_gram_wide_ws_size():
    L, p, _keep = _setup()
    for m in range(1, WIDE_MAX + 1):
        assert L.clhip_gem_gram_wide_ws(m) > 0, m
        assert L.clhip_gem_gram_wide_ws(m) == GRAM_WIDE_BLOCKS * _pairs(m) * 256 * 8, m
    for m in (0, -1, 65, 66, 1 << 20, -(1 << 20)):
        assert L.clhip_gem_gram_wide_ws(m) == 0, m


def test_gram_wide_rejects_bad_arguments():
    L, p, _keep = _setup()
    idx = _idx()
    big = L.clhip_gem_gram_wide_ws(WIDE_MAX)
    # (G, ld, row_idx, m, n, out, ws, ws_bytes, stream)
    good = [p, 8, idx, 20, 8, p, p, big, None]
    for null in (0, 2, 5, 6):
        a = list(good)
        a[null] = None
        assert L.clhip_gem_gram_wide(*a) == EINVAL, null
    for m in (0, -1, 65, 1 << 20):
        a = list(good)
        a[3] = m
        assert L.clhip_gem_gram_wide(*a) == EINVAL, m
    a = list(good)
    a[4] = 0
    assert L.clhip_gem_gram_wide(*a) == EINVAL
    for m in range(1, WIDE_MAX + 1):
        a = list(good)
        a[3], a[7] = m, L.clhip_gem_gram_wide_ws(m) - 1
        assert L.clhip_gem_gram_wide(*a) == EINVAL, m


def test_project_wide_rejects_bad_arguments():
    L, p, _keep = _setup()
    idx = _idx()
    v = (C.c_float * WIDE_MAX)(*([0.5] * WIDE_MAX))
    # (G, ld, row_idx, v_host, m, g, out, n, stream)
    good = [p, 8, idx, v, 20, p, p, 8, None]
    for null in (0, 2, 3, 5, 6):
        a = list(good)
        a[null] = None
        assert L.clhip_gem_project_wide(*a) == EINVAL, null
    for m in (0, -1, 64, 65, 1 << 20):                     # 63 memory rows at the most: the 64th row of a Gram matrix is the gradient
        a = list(good)
        a[4] = m
        assert L.clhip_gem_project_wide(*a) == EINVAL, m
    a = list(good)
    a[7] = 0
    assert L.clhip_gem_project_wide(*a) == EINVAL


def test_project_dev_wide_rejects_bad_arguments():
    L, p, _keep = _setup()
    idx = _idx()
    # (G, ld, row_idx, v_dev, info_dev, m, g, out, n, stream)
    good = [p, 8, idx, p, p, 20, p, p, 8, None]
    for null in (0, 2, 3, 4, 6, 7):
        a = list(good)
        a[null] = None
        assert L.clhip_gem_project_dev_wide(*a) == EINVAL, null
    for m in (0, -1, 64, 65, 1 << 20):
        a = list(good)
        a[5] = m
        assert L.clhip_gem_project_dev_wide(*a) == EINVAL, m
    a = list(good)
    a[8] = 0
    assert L.clhip_gem_project_dev_wide(*a) == EINVAL


def test_more_than_64_tasks_are_refused_at_construction():
    """GemNet and the trainer name the limit before anything is built or loaded, not in the first observe of task 65."""
    import pytest
    from clsurvey_amd.methods import gem_main
    from clsurvey_amd.methods.gem import GemNet
    assert GemNet.MAX_TASKS == WIDE_MAX
    with pytest.raises(ValueError, match="64"):
        GemNet(None, 65, 65, [1] * 65, 1, 1e-2)
    with pytest.raises(ValueError, match="64"):
        gem_main.main(dict(method="gem", n_tasks=65, n_outputs=65, task_count=2, prev_model_path="/nonexistent"), [1] * 65)


def test_qp_wide_rejects_bad_arguments():
    L, p, _keep = _setup()
    margin, eps = C.c_double(0.5), C.c_double(1e-3)
    # (gram, m, margin, eps, v_out, info, ws, ws_bytes, stream); m = memory rows + 1, so m = 2 is the smallest problem and 64 the largest
    for m in range(-1, WIDE_MAX + 2):
        need = L.clhip_gem_qp_wide_ws(m)
        assert need >= 0 and (need == 0 or 2 <= m <= WIDE_MAX), m
    for null in (0, 4, 5):
        a = [p, 20, margin, eps, p, p, p, L.clhip_gem_qp_wide_ws(20), None]
        a[null] = None
        assert L.clhip_gem_qp_wide(*a) == EINVAL, null
    for m in (1, 0, -1, 65, 1 << 20):
        assert L.clhip_gem_qp_wide(p, m, margin, eps, p, p, p, 1 << 20, None) == EINVAL, m
    for m in (2, 17, WIDE_MAX):                            # a workspace shorter than reported (none is needed when it reports 0)
        need = L.clhip_gem_qp_wide_ws(m)
        if need:
            assert L.clhip_gem_qp_wide(p, m, margin, eps, p, p, p, need - 1, None) == EINVAL, m
            assert L.clhip_gem_qp_wide(p, m, margin, eps, p, p, None, need, None) == EINVAL, m
