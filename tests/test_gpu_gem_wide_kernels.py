"""Kernel-level parity of csrc/gem_wide.hip: clhip_gem_gram_wide, clhip_gem_project_wide, clhip_gem_project_dev_wide,
clhip_gem_qp_wide and the chain gram_wide -> qp_wide -> project_dev_wide, called with raw pointers, with the arena and
sentinel discipline, the data and the references of tests/test_gpu_gem_kernels.py (gram_rows, gram_reference, proj_data,
project_reference, chain_problem, Guarded, Arena), whose bounds carry over unchanged:

  gram     per entry |dev - longdouble| <= n 2^-53 sum |terms| (products of two float32 are exact in f64; what is left is the order
           of n f64 additions, whatever the order: matrix-core tiles here).  Bitwise symmetric, two calls bitwise equal, the
           workspace written exactly up to blocks * pairs * 256 doubles (<= what clhip_gem_gram_wide_ws reports) and untouched
           behind, NaN patterns in the unselected row and the padding columns never reach the output.  At m <= 16 the wide entry
           meets the same bound as the narrow one (another order of additions: the two are not compared bit for bit).
  project  bitwise the numpy float64 loop in row order rounded once; project_dev_wide is bitwise project_wide on float32(v);
           info[0] == 0 leaves g untouched and reads no memory row (Inf / NaN planted there).
  qp       the random recipe of test_gpu_parity.py::test_gem_qp_on_device_vs_host_and_scipy with t = 16 .. 63 unknowns and kinds
           0 (d = 3 t + 2), 1 (d = t - 2: rank deficient, only eps I keeps P definite; this is what makes the active set drop
           constraints) and 3 (d = t + 1), margins 0 / 0.5 / 1, 90 cases; the project's tolerances: |v_dev - v_host| <= 1e-9 max(1,
           |v_host|) against oracle/qp_ref.py and the KKT residual <= 1e-10 max(1, |q|_inf, |P|_inf max(1, |v|)).  Kind 2 (near-
           collinear rows, cond(P) ~ 1e8 and more) is LEFT OUT above 15 unknowns: there the host restatement itself is more than
           1e10 times the 1e-9 bound away from a second f64 solve on its own active set, so it is no reference at these sizes;
           for kinds 0, 1 and 3 it stays more than 100 times inside both bounds.
  chain    pinned problems on the grid k / 16: the Gram matrix is exact in f64 in any order (asserted: 0 against longdouble), so
           the device solves the QP of exactly the matrix the host sees; v at 1e-9 max(1, |v|), the projected gradient bitwise
           from the device's own v.  "margin-boundary" at t = 63 ends with 61 constraints active (asserted on both sides).

Every check prints `MEASURED|case|what|device/bound|...` before it asserts (run with -s).  Measured on one MI355X:
  gram (worst entry of any case, device / bound)   row_counts 2.5e-03, short_rows 0.486, scalar_path 0.373, second_trip 1.1e-05
  project_wide, project_dev_wide                   0 ulp in all 3 m x 5 n x 5 paths x 2 (in place or not)
  qp                                               90 solved of 90; worst |v_dev - v_host| / bound 3.3e-03, worst KKT residual / bound 1.6e-02
  chain                                            Gram error 0; |v_dev - v_host| / bound: all-violated <= 4.1e-06, identical-rows <= 3.8e-02,
                                                   margin-boundary <= 1.2e-06; projected gradient 0 ulp
  Run time: 49 tests in 3.4 s, 0.25 s for the slowest.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_parity import Arena, bitwise_equal, ulp_distance
from test_gpu_gem_kernels import (NAN64_BITS, OUT_BITS, PROJ_PATHS, Guarded, chain_problem, dev, gram_reference, gram_rows, lib,
                                  nan_fill, np_bits_equal, proj_data, project_reference, stream)

pytestmark = pytest.mark.gpu

WIDE_CAP = 1024          # block cap of the wide Gram pass (GRAM_WIDE_BLOCKS of csrc/gem_wide.hip)
BLOCK_COLS = 128         # columns a block consumes per trip: 4 waves x 32, on the 16-byte and on the scalar path alike
TILE = 256               # doubles per block and panel pair in the workspace


def wide_pairs(m):
    panels = (m + 15) // 16
    return panels * (panels + 1) // 2


def wide_blocks(n):
    return min(WIDE_CAP, (n + BLOCK_COLS - 1) // BLOCK_COLS)


# ===================================================================================================== clhip_gem_gram_wide
def run_gram_wide(G, sel, n, ld, mis):
    m = len(sel)
    L = lib()
    ar = Arena()
    kg = ar.add(torch.from_numpy(G), misaligned=mis)
    ar.upload(dev())
    need = L.clhip_gem_gram_wide_ws(m)
    assert need == WIDE_CAP * wide_pairs(m) * TILE * 8
    ws = Guarded(torch.float64, need // 8 + 64, fill_bits=NAN64_BITS)
    idx = (C.c_int * m)(*sel)
    outs = []
    for _ in range(2):
        out = Guarded(torch.float64, m * m, fill_bits=NAN64_BITS)
        rc = L.clhip_gem_gram_wide(ar.ptr(kg), ld, idx, m, n, out.ptr, ws.ptr, need, stream())
        torch.cuda.synchronize()
        assert rc == 0
        outs.append(out.get())
    ar.download()
    assert ar.gaps_untouched() and bitwise_equal(ar.get(kg), torch.from_numpy(G).reshape(-1)), "a gap was written or G changed"
    assert torch.equal(outs[0][1], outs[1][1]), "two calls differ"
    return outs[0][0].numpy().reshape(m, m).copy(), ws.get()[0].numpy().copy()


def check_gram_wide(case, m, n, ld, mis=False, seed=0):
    G, sel = gram_rows(m, n, ld, 1000 * m + n % 9973 + seed)
    vec = (not mis) and ld % 4 == 0
    got, ws = run_gram_wide(G, sel, n, ld, mis)
    ref, terms = gram_reference(G, sel, n)
    assert bool(np.isfinite(got).all()), "non-finite Gram entry: a column past n, an unselected row or stale workspace was read"
    assert np_bits_equal(got, got.T.copy()), "the output is not bitwise symmetric"
    bound = np.maximum(n * 2.0 ** -53 * terms, np.finfo(np.float64).tiny)
    r_dev = float((np.abs(got.astype(np.longdouble) - ref) / bound).max())
    print("MEASURED|%s|gram_wide m=%d n=%d ld=%d %s|%.3e" % (case, m, n, ld, "vec" if vec else "scalar", r_dev))
    assert r_dev <= 1.0, "m=%d n=%d: %.3e of n 2^-53 sum|terms|" % (m, n, r_dev)
    if m >= 2 and n >= 64:
        assert abs(ref[0, 1]) <= 1e-4 * terms[0, 1], "the cancelling pair does not cancel: the inputs do not suit the test"
    written = wide_blocks(n) * wide_pairs(m) * TILE
    assert bool(np.isfinite(ws[:written]).all()), "a tile of the first blocks * pairs was not written"
    assert bool((ws[written:].view(np.int64) == np.int64(NAN64_BITS)).all()), "the workspace was written behind blocks * pairs * 256 doubles"


@pytest.mark.parametrize("m", [1, 16, 17, 31, 32, 33, 48, 49, 63, 64])
def test_gram_wide_row_counts(request, m):
    """Every panel count and the row counts around a panel edge at n = 1027 (ld = 1032: 16-byte path, ragged last group), rows
    permuted; m <= 16 is the one-panel instance, held to the narrow entry's bound."""
    check_gram_wide(request.node.name, m, 1027, 1032)


@pytest.mark.parametrize("m", [17, 64])
def test_gram_wide_short_rows(request, m):
    """n around one 8-column group and one 32-column wave trip."""
    for n in (1, 3, 4, 5, 63, 64, 65):
        check_gram_wide(request.node.name, m, n, (n + 3) // 4 * 4 + 4)


@pytest.mark.parametrize("m", [17, 33, 64])
def test_gram_wide_scalar_path(request, m):
    """The scalar loads, reached by a row stride that is no multiple of 4 and by a base one float past 16 bytes."""
    for n in (5, 1027):
        ld = n + 5 if (n + 5) % 4 else n + 6
        assert ld % 4
        check_gram_wide(request.node.name, m, n, ld, seed=1)
        check_gram_wide(request.node.name, m, n, (n + 3) // 4 * 4 + 4, mis=True, seed=2)


@pytest.mark.parametrize("path", ["vec", "scalar"])
def test_gram_wide_second_trip(request, path):
    """The grid is min(1024, ceil(n / 128)) blocks on both load paths (one grid shape): n = 1024 * 128 + 1 is the smallest n at
    which the capped grid takes a second trip (wave 0 of block 0 comes round for one column).  m = 17: G stays at 9 MB."""
    n = WIDE_CAP * BLOCK_COLS + 1
    assert wide_blocks(n) == WIDE_CAP and wide_blocks(n - 1) == WIDE_CAP and (n - 1) // BLOCK_COLS == WIDE_CAP
    ld = (n + 3) // 4 * 4 + 4 if path == "vec" else n + 5
    assert (ld % 4 == 0) == (path == "vec")
    check_gram_wide(request.node.name, 17, n, ld)


# ================================================================= clhip_gem_project_wide / clhip_gem_project_dev_wide
def run_project_wide(G, sel, ld, n, g, v, info=None, inplace=False, mis_G=False, mis_g=False, mis_out=False, ld_odd=False):
    """info None: clhip_gem_project_wide with host float32 v; else clhip_gem_project_dev_wide with v as f64 and info on the
    device.  Returns (out, g afterwards)."""
    L = lib()
    m = len(sel)
    ar = Arena()
    kG = ar.add(torch.from_numpy(G), misaligned=mis_G)
    kg = ar.add(torch.from_numpy(g), misaligned=mis_g or (inplace and mis_out))
    ko = kg if inplace else ar.add(n, misaligned=mis_out, fill=OUT_BITS)
    ar.upload(dev())
    idx = (C.c_int * m)(*sel)
    if info is None:
        rc = L.clhip_gem_project_wide(ar.ptr(kG), ld, idx, (C.c_float * m)(*[float(x) for x in v]), m, ar.ptr(kg), ar.ptr(ko), n, stream())
    else:
        vd = Guarded(torch.float64, m, init=torch.from_numpy(np.asarray(v, np.float64)))
        nd = Guarded(torch.int32, 2, init=torch.tensor(info, dtype=torch.int32))
        rc = L.clhip_gem_project_dev_wide(ar.ptr(kG), ld, idx, vd.ptr, nd.ptr, m, ar.ptr(kg), ar.ptr(ko), n, stream())
    torch.cuda.synchronize()
    ar.download()
    assert rc == 0 and ar.gaps_untouched(), "rc %d or a gap was written" % rc
    assert bitwise_equal(ar.get(kG), torch.from_numpy(G).reshape(-1)), "G changed"
    if info is not None:
        assert np_bits_equal(vd.get()[0].numpy(), np.asarray(v, np.float64)), "v changed"
        assert nd.get()[0].tolist() == list(info), "info changed"
    if not inplace:
        assert np_bits_equal(ar.get(kg).numpy(), g), "g changed by an out-of-place call"
    return ar.get(ko).numpy().copy(), ar.get(kg).numpy().copy()


@pytest.mark.parametrize("path", list(PROJ_PATHS))
@pytest.mark.parametrize("m", [17, 32, 63])
def test_project_wide_and_project_dev_wide(request, m, path):
    kw = PROJ_PATHS[path]
    for n in (1, 3, 4, 5, 1027):
        G, sel, ld, g, v64 = proj_data(m, n, bool(kw.get("ld_odd")))
        v32 = v64.astype(np.float32)
        assert not np.array_equal(v32.astype(np.float64), v64)
        want = project_reference(G, sel, n, g, v32)
        for inplace in (False, True):
            what = "m=%d n=%d %s %s" % (m, n, path, "in-place" if inplace else "out-of-place")
            out, _ = run_project_wide(G, sel, ld, n, g, v32, inplace=inplace, **kw)
            ulps = ulp_distance(torch.from_numpy(out), torch.from_numpy(want))
            print("MEASURED|%s|project_wide %s ulp|%d|0" % (request.node.name, what, ulps))
            assert np_bits_equal(out, want), "project_wide %s: %d ulp from the float64 loop rounded once" % (what, ulps)
            outd, _ = run_project_wide(G, sel, ld, n, g, v64, info=(2, 0), inplace=inplace, **kw)
            ulps = ulp_distance(torch.from_numpy(outd), torch.from_numpy(want))
            print("MEASURED|%s|project_dev_wide %s ulp|%d|0" % (request.node.name, what, ulps))
            assert np_bits_equal(outd, want), "project_dev_wide %s: %d ulp from the float64 loop on float32(v)" % (what, ulps)
            assert np_bits_equal(outd, out), "project_dev_wide differs from project_wide given float32(v)"
            out0, g0 = run_project_wide(G, sel, ld, n, g, v64, info=(0, 0), inplace=inplace, **kw)
            assert np_bits_equal(g0, g), "info[0] = 0: g changed"
            assert np_bits_equal(out0, g), "info[0] = 0: out is not g bit for bit"


@pytest.mark.parametrize("path", ["aligned", "ld%4"])
@pytest.mark.parametrize("m", [17, 63])
def test_project_dev_wide_unviolated_ignores_the_memory(request, m, path):
    """info[0] == 0 and out != g: out is g bit for bit with Inf / NaN inside the memory rows; violated, the poison reaches
    exactly its columns."""
    kw = PROJ_PATHS[path]
    for n in (5, 1027):
        G, sel, ld, g, v64 = proj_data(m, n, bool(kw.get("ld_odd")))
        G = G.copy()
        G[sel[0], 0] = np.inf
        G[sel[-1], n - 1] = np.nan
        G[sel[m // 2], n // 2] = -np.inf
        out, g_after = run_project_wide(G, sel, ld, n, g, v64, info=(0, 0), **kw)
        print("MEASURED|%s|unviolated m=%d n=%d non-finite out|%d|0" % (request.node.name, m, n, int((~np.isfinite(out)).sum())))
        assert np_bits_equal(out, g) and np_bits_equal(g_after, g), "out != g although nothing is violated"
        out, _ = run_project_wide(G, sel, ld, n, g, v64, info=(1, 0), **kw)
        assert sorted(np.nonzero(~np.isfinite(out))[0].tolist()) == sorted({0, n - 1, n // 2})


# ===================================================================================================== clhip_gem_qp_wide
def test_qp_wide_vs_host_restatement():
    """See the file's docstring (qp): 90 random problems, t = 16 .. 63, kinds 0 / 1 / 3 (kind 2 left out above 15 unknowns)."""
    from oracle import qp_ref as qp
    L = lib()
    rs = np.random.RandomState(58)
    gram_d = Guarded(torch.float64, 64 * 64, fill_bits=NAN64_BITS)
    v_d = Guarded(torch.float64, 63, fill_bits=NAN64_BITS)
    info_d = Guarded(torch.int32, 2, fill_bits=-1)
    gram_t = gram_d.dev[Guarded.PAD:Guarded.PAD + 64 * 64].view(torch.float64)
    need = L.clhip_gem_qp_wide_ws(64)
    ws = Guarded(torch.float64, need // 8 + 16, fill_bits=NAN64_BITS)
    solved = skipped = 0
    worst_v = worst_kkt = 0.0
    for case in range(90):
        t = int(rs.randint(16, 64))
        kind = (0, 1, 3)[case % 3]
        d = {0: 3 * t + 2, 1: t - 2, 3: t + 1}[kind]
        M = rs.standard_normal((t, d))
        g = rs.standard_normal(d) * (1.0 if case % 5 else 5.0)
        if case % 7 == 0:
            g = np.abs(M).sum(0)                   # positive correlation with most rows: few / no violations
        margin = [0.0, 0.5, 1.0][(case // 3) % 3]
        rows = np.vstack([M, g[None]])
        gram = rows @ rows.T
        m = t + 1
        gram_t[:m * m].copy_(torch.from_numpy(gram.reshape(-1)))
        rc = L.clhip_gem_qp_wide(gram_d.ptr, m, C.c_double(margin), C.c_double(1e-3), v_d.ptr, info_d.ptr, ws.ptr, need, stream())
        assert rc == 0
        info = info_d.get()[0].tolist()
        v = v_d.get()[0].numpy()[:t].copy()
        viol = int((gram[-1, :-1] < 0).sum())
        assert info[0] == viol and info[1] == 0, (case, t, kind, info, viol)
        if viol == 0:
            assert not v.any()
            skipped += 1
            continue
        P = 0.5 * (gram[:t, :t] + gram[:t, :t].T) + 1e-3 * np.eye(t)
        q = -gram[:t, t]
        v_host = qp.project2cone2_coefficients(gram, t, list(range(t)), margin)
        scale = max(1.0, float(np.abs(v_host).max()))
        r_v = float(np.abs(v - v_host).max()) / (1e-9 * scale)
        lam = P @ v - q                                  # multipliers of v >= margin
        kkt = max(float(np.maximum(margin - v, 0).max()), float(np.maximum(-lam, 0).max()), float(np.abs(lam * (v - margin)).max()))
        r_kkt = kkt / (1e-10 * max(1.0, float(np.abs(q).max()), float(np.abs(P).sum(1).max()) * scale))
        print("MEASURED|qp_wide|case %d t=%d kind=%d margin=%g viol=%d|%.3e|%.3e" % (case, t, kind, margin, viol, r_v, r_kkt))
        assert r_v <= 1.0, (case, t, kind, r_v)
        assert r_kkt <= 1.0, (case, t, kind, r_kkt)
        worst_v, worst_kkt = max(worst_v, r_v), max(worst_kkt, r_kkt)
        solved += 1
    ws.get()
    print("MEASURED|qp_wide|solved %d skipped %d|%.3e|%.3e" % (solved, skipped, worst_v, worst_kkt))
    assert solved >= 60, (solved, skipped)


# ===================================================================================================== the chain
@pytest.mark.parametrize("t", [16, 17, 32, 63])
@pytest.mark.parametrize("kind", ["all-violated", "identical-rows", "margin-boundary"])
def test_chain_wide_gram_qp_project(request, kind, t):
    from oracle import qp_ref
    L = lib()
    n, ld, m = 1027, 1032, t + 1
    M, g, margin = chain_problem(kind, t, n)
    G = nan_fill(np.empty((m + 1, ld), np.float32))
    order = list(range(1, t + 1))                         # memory rows 1 .. t, the gradient in row t + 1, row 0 unused
    G[1:t + 1, :n], G[t + 1, :n] = M, g
    sel = order + [t + 1]
    ref, terms = gram_reference(G, sel, n)
    gram64 = ref.astype(np.float64)
    assert np.array_equal(gram64.astype(np.longdouble), ref), "the pinned problem's Gram matrix is not exact in float64"
    viol = int((gram64[t, :t] < 0).sum())
    v_host = qp_ref.project2cone2_coefficients(gram64, t, list(range(t)), margin)
    at_margin = int((np.abs(v_host - margin) <= 1e-9).sum())
    if kind == "all-violated":
        assert viol == t
    elif kind == "identical-rows":
        assert viol > 0 and np.array_equal(gram64[0], gram64[t // 2])
    else:
        assert viol > 0 and at_margin >= 1 and int((v_host > margin + 1e-3).sum()) >= 1, v_host
        if t == 63:
            assert at_margin == 61                        # the outer loop of the active-set method really runs long
    ar = Arena()
    kG = ar.add(torch.from_numpy(G))
    ko = ar.add(n, fill=OUT_BITS)
    ar.upload(dev())
    need = L.clhip_gem_gram_wide_ws(m)
    ws = Guarded(torch.float64, need // 8, fill_bits=NAN64_BITS)
    qneed = L.clhip_gem_qp_wide_ws(m)
    qws = Guarded(torch.float64, qneed // 8 + 16, fill_bits=NAN64_BITS)
    gram = Guarded(torch.float64, m * m, fill_bits=NAN64_BITS)
    v = Guarded(torch.float64, t, fill_bits=NAN64_BITS)
    info = Guarded(torch.int32, 2, fill_bits=-1)
    s = stream()
    g_ptr = ar.ptr(kG) + 4 * (t + 1) * ld
    assert L.clhip_gem_gram_wide(ar.ptr(kG), ld, (C.c_int * m)(*sel), m, n, gram.ptr, ws.ptr, need, s) == 0
    assert L.clhip_gem_qp_wide(gram.ptr, m, C.c_double(margin), C.c_double(1e-3), v.ptr, info.ptr, qws.ptr, qneed, s) == 0
    assert L.clhip_gem_project_dev_wide(ar.ptr(kG), ld, (C.c_int * t)(*order), v.ptr, info.ptr, t, g_ptr, ar.ptr(ko), n, s) == 0
    torch.cuda.synchronize()                              # the only host contact of the chain
    ar.download()
    assert ar.gaps_untouched() and bitwise_equal(ar.get(kG), torch.from_numpy(G).reshape(-1))
    ws.get(), qws.get()
    gram_dev = gram.get()[0].numpy().reshape(m, m)
    err_gram = float(np.abs(gram_dev.astype(np.longdouble) - ref).max())
    v_dev = v.get()[0].numpy().copy()
    assert info.get()[0].tolist() == [viol, 0]
    scale = max(1.0, float(np.abs(v_host).max()))
    r_v = float(np.abs(v_dev - v_host).max()) / (1e-9 * scale)
    print("MEASURED|%s|gram abs error|%.3e|0" % (request.node.name, err_gram))
    print("MEASURED|%s|v (max |v| %.3g, %d at the margin)|%.3e|0" % (request.node.name, scale, at_margin, r_v))
    assert err_gram == 0.0, "the device Gram matrix of the pinned problem is not exact"
    assert r_v <= 1.0, r_v
    if kind == "margin-boundary" and t == 63:
        assert int((np.abs(v_dev - margin) <= 1e-9).sum()) == 61
    want = project_reference(G, order, n, g, v_dev.astype(np.float32))
    out = ar.get(ko).numpy()
    ulps = ulp_distance(torch.from_numpy(out.copy()), torch.from_numpy(want))
    print("MEASURED|%s|projected gradient ulp|%d|0" % (request.node.name, ulps))
    assert np_bits_equal(out, want), "%d ulp from the float64 loop on the device's own float32(v)" % ulps
    assert float(np.abs(v_dev).max()) > 0 and not np_bits_equal(out, g)
