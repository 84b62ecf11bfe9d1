"""Kernel-level parity of csrc/gem.hip: clhip_axpy, clhip_gem_gram, clhip_gem_project, clhip_gem_project_dev and the chain
gram -> clhip_gem_qp -> project_dev, called with raw pointers.  The float operands of a call live in one kernel_parity.Arena
(sentinel gaps between them); the f64 and int buffers (Gram output, workspace, v, info) are Guarded tensors with sentinel
pads of their own.  After every call the gaps and pads are untouched and inputs that are only read are bitwise unchanged.

Bounds, each derived (u = 2^-24, the unit roundoff of float32):
  axpy       alpha in {1, -1, 0.5, 2}: alpha * x is exact, so y + alpha * x is ONE rounding whether or not the compiler contracts the
             multiply-add: bitwise numpy float32 (alpha * x bitwise under assign).  General alpha (0.3, -1.7): unfused,
             fl(fl(alpha x) + y) is off by at most u |alpha x| + u |y + fl(alpha x)| <= 2u (|y| + |alpha x|); fused, by u |y + alpha x|.
             Asserted per element: |dev - fp64| <= 2^-23 (|y| + |alpha x|), on data whose every third y is -fl(alpha x); numpy's unfused
             float32 has to meet it too.  With assign = 1, y starts as a NaN pattern and must not be read.
  gram       a product of two float32 has 48 significant bits and is exact in f64; what is left is the order of n f64 additions,
             (n - 1) 2^-53 sum_c |G_i[c] G_j[c]| for any order.  Asserted per entry with the factor n against the numpy longdouble sum of the
             exact products.  Columns n .. ld-1 of every row and the one row of G that is not selected hold a NaN pattern, the
             workspace starts from a NaN pattern; rows span 2^-20 .. 2^20 and one selected pair cancels to < 1e-4 of its sum of
             magnitudes (asserted), where a fixed fraction of max|ref| sees nothing.  The last column of the table below is a
             float32 accumulator (numpy.dot on the float32 rows) against the same bound: 1e4 .. 1e6 times over it.
  project    s = f64(g[c]); s += f64(v_i) * f64(G_i[c]) in row order; every product is exact (24 + 24 bits), every add is one f64
             rounding in a fixed order, one rounding to float32 at the end: BITWISE the numpy float64 loop, with or without
             contraction.  project_dev rounds its f64 v to float32 first (as torch.Tensor(v) does in gem.py) and is then bitwise
             clhip_gem_project on that float32 v; with info[0] == 0 the result is g, bit for bit, in place or not.
  chain      pinned problems on the grid k / 16: every Gram entry is then exact in f64 in ANY summation order (device Gram against
             the longdouble one: measured 0), so clhip_gem_qp solves the QP of exactly the matrix oracle/qp_ref.py sees and the
             tolerance of test_gem_qp_on_device_vs_host_and_scipy applies: |v_dev - v_host| <= 1e-9 max(1, |v|).  The projected
             gradient is judged by the bitwise rule from the device's own v.

Measured on one MI355X (every check prints `MEASURED|case|what|device/bound|reference/bound` before it asserts; run with -s):
  axpy, exact alphas, 8 lengths x 3 alignments x 2 assign      0 ulp from numpy float32 everywhere
  axpy, alpha 0.3 / -1.7 (worst element of any case)            assign 0: 0.499 / numpy float32 0.957;  assign 1: 0.485 / 0.485
                                                                (0.499 < 0.5: the device contracts the multiply-add, numpy does not)
  gram (worst entry of any case)                                device / bound    float32 accumulator / bound (smallest)
    every_row_count  m = 1 .. 16, n = 1027, ld = 1032           2.3e-03           2.2e+05
    short_rows       m = 3, 12, 16, n = 1 .. 65                 0.374             4.5e+06
    scalar_path      ld % 4 != 0, G one float off               0.204             2.6e+05
    second_stride_trip  S1-m2 / S2-m12 / S4-m16                 1.0e-07 / 7.4e-07 / 1.8e-06     1.3e+04
  project, project_dev: 0 ulp in all 4 m x 5 n x 5 paths x 2 (in place or not) and the 10 second-trip cases
  chain: Gram 0 / bound; |v_dev - v_host| / (1e-9 max(1, |v|)): all-violated 2.1e-06 (t = 15), 4.7e-07 (t = 4); identical-rows
         1.5e-02, 1.1e-02; margin-boundary 2.1e-07, 1.1e-07; projected gradient 0 ulp
  Run time on the MI355X: 89 tests in 6.3 s; 0.83 s for the slowest (second_stride_trip[S2-m12]: a 100 MB G and its longdouble reference).

Bug found by reading and fixed with this file: project_dev_kernel with info[0] == 0 and out != g computed g + 0.0 * G[row]; an
Inf / NaN inside a memory row turned out into NaN where gem.py:275-277 leaves the gradient alone.  A library built from the
kernel before the fix fails test_project_dev_unviolated_ignores_the_memory in all 6 cases and nothing else of this file.

Mutation check, run once against scratch copies of gem.hip (each mutant only reads less or other in-bounds memory, none writes
elsewhere; one run of this file per mutant with CLHIP_LIB on the mutant library; not part of the repository):
  (a) gram accumulator rounded to float32 at every add      26 fail: gram_every_row_count x16, gram_scalar_path x6, gram_short_rows x3,
                                                            gram_second_stride_trip[S4-m16].  [S1-m2] and [S2-m12] pass: a thread adds
                                                            only ~10 products there before the f64 tree takes over, and the worst-case
                                                            bound grows like n^2 mean|term| (n = 2 .. 4 million) while those few float32
                                                            roundings do not; the small-n tests are the ones that see this mutant
  (b) gram: n4 computed from ld instead of n                28 fail: gram_every_row_count x16, gram_short_rows x3, second_stride_trip x3 (the
                                                            NaN columns are read), chain x6.  Not gram_scalar_path: n4 is 0 there
  (c) gram: stride gridDim * GB instead of gridDim * COLS   2 fail: gram_second_stride_trip[S2-m12] and [S4-m16], 2e9 / 4e9 times the bound.
                                                            [S1-m2] passes and must: COLS == GB for S = 1, the mutant is the product there
  (d) project rounds v * G to float32 before the add        25 fail: project_and_project_dev x20, project_second_stride_trip x5
  (e) project_dev without the float32 rounding of v         31 fail: project_and_project_dev x20, project_second_stride_trip x5, chain x6
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from kernel_parity import Arena, bitwise_equal, ulp_distance

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF             # padding columns, unused rows, outputs before a call: a quiet NaN with a payload
OUT_BITS = 0x7FC00A11
NAN64_BITS = 0x7FF80000DEADBEEF   # the f64 workspace / outputs before a call
PAD64_BITS = 0x4045000000000000   # 42.0: the pads around an f64 buffer
PAD32_BITS = 0x00A5A5A5           # the pads around an int32 buffer
GB = 256                          # threads per block of every kernel of the file
CAP = 2048                        # ew_grid's / the Gram pass's block cap
BIG_AXPY = CAP * GB * 4 + 1027    # > 2048 * 256 float4: the 16-byte loop takes a second trip (the scalar loop a fifth)


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def lib():
    from clsurvey_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_fill(a, bits=NAN_BITS):
    """Fill a float32 numpy view with the NaN pattern, bit for bit."""
    a.view(np.int32)[...] = bits
    return a


def np_bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


class Guarded:
    """n elements of float64 / int32 on the device between two pads of 16 sentinel elements."""
    PAD = 16

    def __init__(self, dtype, n, init=None, fill_bits=None):
        self.dtype, self.n = dtype, int(n)
        self.ityp, self.pad_bits = (torch.int64, PAD64_BITS) if dtype == torch.float64 else (torch.int32, PAD32_BITS)
        host = torch.full((self.n + 2 * self.PAD,), self.pad_bits, dtype=self.ityp)
        mid = host[self.PAD:self.PAD + self.n]
        if init is not None:
            mid.copy_(torch.as_tensor(init, dtype=dtype).reshape(-1).view(self.ityp))
        else:
            mid.fill_(fill_bits if fill_bits is not None else 0)
        self.dev = host.to(dev())
        self.ptr = self.dev.data_ptr() + self.PAD * self.dev.element_size()
        self.nbytes = self.n * self.dev.element_size()

    def get(self):
        """(values, their bit patterns) on the host; asserts that the pads are untouched."""
        back = self.dev.cpu()
        pads = torch.cat([back[:self.PAD], back[self.PAD + self.n:]])
        assert bool((pads == self.pad_bits).all()), "a pad around an f64 / int buffer was written"
        mid = back[self.PAD:self.PAD + self.n].clone()
        return mid.view(self.dtype), mid


# ===================================================================================================== clhip_axpy
AXPY_N = [1, 3, 4, 5, 255, 1024, 1027, BIG_AXPY]
AXPY_PATHS = {"aligned": (False, False), "x-off": (True, False), "y-off": (False, True)}     # (x, y) one float past 16 bytes


@functools.lru_cache(maxsize=None)
def axpy_data(n, alpha):
    """x, y with every third y = -fl(alpha * x) (the sum cancels), magnitudes over 2^+-10."""
    rs = np.random.RandomState(n % 100003 + 17)
    x = (rs.standard_normal(n) * np.exp2(rs.randint(-10, 11, size=n))).astype(np.float32)
    y = (rs.standard_normal(n) * np.exp2(rs.randint(-10, 11, size=n))).astype(np.float32)
    y[::3] = -(np.float32(alpha) * x[::3])
    return x, y


def run_axpy(x, y, alpha, assign, mis_x, mis_y):
    ar = Arena()
    kx = ar.add(torch.from_numpy(x), misaligned=mis_x)
    ky = ar.add(torch.from_numpy(y), misaligned=mis_y)
    ar.upload(dev())
    assert ar.ptr(kx) % 16 == (4 if mis_x else 0) and ar.ptr(ky) % 16 == (4 if mis_y else 0)
    rc = lib().clhip_axpy(ar.ptr(ky), ar.ptr(kx), x.size, alpha, assign, stream())
    torch.cuda.synchronize()
    ar.download()
    assert rc == 0 and ar.gaps_untouched(), "rc %d or a gap was written" % rc
    assert np_bits_equal(ar.get(kx).numpy(), x), "x changed"
    return ar.get(ky).numpy().copy()


@pytest.mark.parametrize("path", list(AXPY_PATHS))
@pytest.mark.parametrize("n", AXPY_N)
def test_axpy(request, n, path):
    """y = y + alpha x (assign 0) / y = alpha x (assign 1, y never read: it starts as NaN): bitwise numpy float32 for the
    alphas whose product is exact, the derived bound for general ones, non-finite x stays in its own element."""
    case = request.node.name
    mis_x, mis_y = AXPY_PATHS[path]
    u23 = 2.0 ** -23
    for assign in (0, 1):
        for alpha in (1.0, -1.0, 0.5, 2.0, 0.3, -1.7):
            if n == BIG_AXPY and alpha not in (0.5, 0.3):
                continue                                   # the large length: one exact and one general alpha per path
            a32 = np.float32(alpha)
            x, y = axpy_data(n, alpha)
            y0 = nan_fill(np.empty(n, np.float32), OUT_BITS) if assign else y
            got = run_axpy(x, y0, alpha, assign, mis_x, mis_y)
            assert bool(np.isfinite(got).all()), "assign=%d alpha=%g: non-finite output (y read under assign, or unwritten)" % (assign, alpha)
            want32 = a32 * x if assign else y + a32 * x                  # numpy float32, unfused
            want64 = float(a32) * x.astype(np.float64) + (0.0 if assign else y.astype(np.float64))
            what = "assign%d alpha=%g" % (assign, alpha)
            if alpha in (1.0, -1.0, 0.5, 2.0):
                ulps = ulp_distance(torch.from_numpy(got), torch.from_numpy(want32))
                print("MEASURED|%s|%s ulp|%d|0" % (case, what, ulps))
                assert np_bits_equal(got, want32), "%s: %d ulp from numpy float32" % (what, ulps)
            else:
                terms = np.abs(float(a32) * x.astype(np.float64)) + (0.0 if assign else np.abs(y.astype(np.float64)))
                bound = np.maximum(u23 * terms, np.finfo(np.float64).tiny)
                r_dev = float((np.abs(got.astype(np.float64) - want64) / bound).max())
                r_cpu = float((np.abs(want32.astype(np.float64) - want64) / bound).max())
                print("MEASURED|%s|%s|%.3f|%.3f" % (case, what, r_dev, r_cpu))
                assert r_cpu <= 1.0, "numpy float32 misses the bound: the inputs do not suit the rule"
                assert r_dev <= 1.0, "%s: %.3f of 2^-23 (|y| + |alpha x|)" % (what, r_dev)
        # a non-finite x element reaches exactly its own position (first, last, and one in the 16-byte body / tail)
        x, y = axpy_data(n, 0.5)
        clean = run_axpy(x, y, 0.5, assign, mis_x, mis_y) if n != BIG_AXPY else None
        if clean is not None:
            for pos, val in ((0, np.inf), (n - 1, np.nan), (n // 2, -np.inf)):
                x2 = x.copy()
                x2[pos] = val
                got = run_axpy(x2, y, 0.5, assign, mis_x, mis_y)
                keep = np.ones(n, bool)
                keep[pos] = False
                assert not np.isfinite(got[pos]) and np_bits_equal(got[keep], clean[keep]), "%r at %d leaked or was lost" % (val, pos)


# ===================================================================================================== clhip_gem_gram
def gram_split(m):
    return 1 if m <= 11 else 2 if m <= 15 else 4


def gram_blocks(m, n, vec):
    work = n // 4 + 1 if vec else n
    per = GB // gram_split(m)
    return min(CAP, max(1, (work + per - 1) // per))


def gram_rows(m, n, ld, seed):
    """G[R][ld] with R = m + 1 rows (m = 1: one row) and the m selected rows in permuted order, first and last row of G among
    them; the row that is not selected and columns n .. ld-1 of every row hold a NaN pattern.  Row magnitudes span 2^-20 ..
    2^20; the second selected row is the first with every odd column's sign flipped, and the odd columns of the first repeat
    the even ones up to 2^-20, so that pair's products cancel to ~1e-6 of the sum of their magnitudes."""
    rs = np.random.RandomState(seed)
    rg = np.random.default_rng(seed)
    R = m + 1 if m > 1 else 1
    G = nan_fill(np.empty((R, ld), np.float32))
    if m == 1:
        sel = [0]
    else:
        mid = list(rs.permutation(np.arange(1, R - 1)))[:m - 2]
        sel = [int(v) for v in rs.permutation([0, R - 1] + mid)]
    expo = rs.permutation(np.linspace(-20, 20, m).round()) if m > 1 else np.zeros(1)
    for k, r in enumerate(sel):
        G[r, :n] = rg.standard_normal(n, dtype=np.float32) * np.float32(2.0 ** expo[k])
    if m >= 2 and n >= 2:
        a = G[sel[0], :n].copy()
        h = n // 2
        a[1:2 * h:2] = a[0:2 * h:2] * (np.float32(1) + np.float32(2.0 ** -20) * rs.randint(-8, 9, size=h).astype(np.float32))
        G[sel[0], :n] = a
        b = a.copy()
        b[1::2] = -b[1::2]
        b[2 * h:] = 0                                        # (odd n: the unpaired last column takes no part)
        G[sel[1], :n] = b * np.float32(2.0 ** 7)
    return G, sel


def gram_reference(G, sel, n):
    """(longdouble Gram matrix, sum of |terms| per entry): products of two float32 are exact in float64."""
    m = len(sel)
    ref = np.zeros((m, m), np.longdouble)
    terms = np.zeros((m, m), np.float64)
    rows = [G[r, :n].astype(np.float64) for r in sel]
    for i in range(m):
        for j in range(i, m):
            prod = rows[i] * rows[j]
            ref[i, j] = ref[j, i] = prod.sum(dtype=np.longdouble)
            terms[i, j] = terms[j, i] = np.abs(prod).sum()
    return ref, terms


def run_gram(G, sel, n, ld, mis):
    m = len(sel)
    L = lib()
    ar = Arena()
    kg = ar.add(torch.from_numpy(G), misaligned=mis)
    ar.upload(dev())
    need = L.clhip_gem_gram_ws(m)
    ws = Guarded(torch.float64, need // 8 + 64, fill_bits=NAN64_BITS)
    idx = (C.c_int * m)(*sel)
    outs = []
    for _ in range(2):
        out = Guarded(torch.float64, m * m, fill_bits=NAN64_BITS)
        rc = L.clhip_gem_gram(ar.ptr(kg), ld, idx, m, n, out.ptr, ws.ptr, need, stream())
        torch.cuda.synchronize()
        assert rc == 0
        outs.append(out.get())
    ar.download()
    assert ar.gaps_untouched() and bitwise_equal(ar.get(kg), torch.from_numpy(G).reshape(-1)), "a gap was written or G changed"
    assert torch.equal(outs[0][1], outs[1][1]), "two calls differ"
    return outs[0][0].numpy().reshape(m, m).copy(), ws.get()[0].numpy().copy()


def check_gram(case, m, n, ld, mis=False, seed=0):
    G, sel = gram_rows(m, n, ld, 1000 * m + n % 9973 + seed)
    vec = (not mis) and ld % 4 == 0
    got, ws = run_gram(G, sel, n, ld, mis)
    ref, terms = gram_reference(G, sel, n)
    assert bool(np.isfinite(got).all()), "non-finite Gram entry: a column past n, an unselected row or stale workspace was read"
    assert np_bits_equal(got, got.T.copy()), "the output is not bitwise symmetric"
    bound = np.maximum(n * 2.0 ** -53 * terms, np.finfo(np.float64).tiny)
    r_dev = float((np.abs(got.astype(np.longdouble) - ref) / bound).max())
    f32 = np.array([[np.dot(G[a, :n], G[b, :n]) for b in sel] for a in sel], np.float64)     # a float32 accumulator, for scale
    r_f32 = float((np.abs(f32.astype(np.longdouble) - ref) / bound).max())
    print("MEASURED|%s|gram m=%d n=%d ld=%d %s|%.3e|%.3e" % (case, m, n, ld, "vec" if vec else "scalar", r_dev, r_f32))
    assert r_dev <= 1.0, "m=%d n=%d: %.3e of n 2^-53 sum|terms|" % (m, n, r_dev)
    if m >= 2 and n >= 64:
        assert abs(ref[0, 1]) <= 1e-4 * terms[0, 1], "the cancelling pair does not cancel: the inputs do not suit the test"
    written = gram_blocks(m, n, vec) * (m * (m + 1) // 2)
    assert bool(np.isfinite(ws[:written]).all()), "a partial of the first blocks * pairs doubles was not written"
    assert bool((ws[written:].view(np.int64) == np.int64(NAN64_BITS)).all()), "the workspace was written behind blocks * pairs doubles"


@pytest.mark.parametrize("m", range(1, 17))
def test_gram_every_row_count(request, m):
    """All 16 template instances at n = 1027 (ld = 1032: 16-byte path, tail of 3), rows permuted."""
    check_gram(request.node.name, m, 1027, 1032)


@pytest.mark.parametrize("m", [3, 12, 16])
def test_gram_short_rows(request, m):
    """n around one column group and one wave, for one m of every split class (S = 1 / 2 / 4)."""
    for n in (1, 2, 3, 4, 5, 63, 64, 65):
        check_gram(request.node.name, m, n, (n + 3) // 4 * 4 + 4)


@pytest.mark.parametrize("m", [1, 3, 11, 12, 15, 16])
def test_gram_scalar_path(request, m):
    """The scalar loop, reached by a row stride that is no multiple of 4 and by a base one float past 16 bytes."""
    for n in (5, 1027):
        ld = n + 5 if (n + 5) % 4 else n + 6
        assert ld % 4
        check_gram(request.node.name, m, n, ld, seed=1)
        check_gram(request.node.name, m, n, (n + 3) // 4 * 4 + 4, mis=True, seed=2)


@pytest.mark.parametrize("m,cols", [(2, 256), (12, 128), (16, 64)], ids=["S1-m2", "S2-m12", "S4-m16"])
def test_gram_second_stride_trip(request, m, cols):
    """n just above 2 * 2048 * (256 / S) * 4 with n % 4 = 3: every block of the capped grid comes round again (stride =
    2048 * 256 / S column groups, not 2048 * 256) and the last trip is ragged."""
    assert cols == GB // gram_split(m)
    n = 2 * CAP * cols * 4 + 1027
    assert n % 4 == 3 and gram_blocks(m, n, True) == CAP and n // 4 > 2 * CAP * cols
    check_gram(request.node.name, m, n, n + 5)


# ============================================================================ clhip_gem_project / clhip_gem_project_dev
PROJ_PATHS = {"aligned": {}, "G-off": dict(mis_G=True), "ld%4": dict(ld_odd=True), "g-off": dict(mis_g=True), "out-off": dict(mis_out=True)}
BIG_PROJ = CAP * GB * 4 + 1027


@functools.lru_cache(maxsize=None)
def proj_data(m, n, ld_odd):
    rs = np.random.RandomState(31 * m + n % 9973 + (7 if ld_odd else 0))
    ld = (n + 3) // 4 * 4 + 4 + (1 if ld_odd else 0)
    R = m + 1
    G = nan_fill(np.empty((R, ld), np.float32))
    sel = [int(v) for v in rs.permutation(R)[:m]]
    if 0 not in sel:
        sel[0] = 0
    for r in sel:
        G[r, :n] = (rs.standard_normal(n) * np.exp2(rs.randint(-6, 7, size=n))).astype(np.float32)
    g = rs.standard_normal(n).astype(np.float32)
    v64 = rs.standard_normal(m) * 1.5 + 1.0 / 3.0                    # no component is a float32
    return G, sel, ld, g, v64


def project_reference(G, sel, n, g, v32):
    """gem.py:79 in numpy float64, rows in the order given, rounded once to float32.  Every product is exact in float64."""
    s = g.astype(np.float64)
    for vi, r in zip(v32, sel):
        s += np.float64(vi) * G[r, :n].astype(np.float64)
    return s.astype(np.float32)


def run_project(G, sel, ld, n, g, v, info=None, inplace=False, mis_G=False, mis_g=False, mis_out=False, ld_odd=False):
    """info None: clhip_gem_project with host float32 v; else clhip_gem_project_dev with v as f64 and info on the device.
    Returns (out, g afterwards)."""
    L = lib()
    m = len(sel)
    ar = Arena()
    kG = ar.add(torch.from_numpy(G), misaligned=mis_G)
    kg = ar.add(torch.from_numpy(g), misaligned=mis_g or (inplace and mis_out))
    ko = kg if inplace else ar.add(n, misaligned=mis_out, fill=OUT_BITS)
    ar.upload(dev())
    idx = (C.c_int * m)(*sel)
    if info is None:
        rc = L.clhip_gem_project(ar.ptr(kG), ld, idx, (C.c_float * m)(*[float(x) for x in v]), m, ar.ptr(kg), ar.ptr(ko), n, stream())
    else:
        vd = Guarded(torch.float64, m, init=torch.from_numpy(np.asarray(v, np.float64)))
        nd = Guarded(torch.int32, 2, init=torch.tensor(info, dtype=torch.int32))
        rc = L.clhip_gem_project_dev(ar.ptr(kG), ld, idx, vd.ptr, nd.ptr, m, ar.ptr(kg), ar.ptr(ko), n, stream())
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


def check_project(case, m, n, path, inplace):
    kw = PROJ_PATHS[path]
    G, sel, ld, g, v64 = proj_data(m, n, bool(kw.get("ld_odd")))
    v32 = v64.astype(np.float32)
    assert not np.array_equal(v32.astype(np.float64), v64)
    want = project_reference(G, sel, n, g, v32)
    what = "m=%d n=%d %s %s" % (m, n, path, "in-place" if inplace else "out-of-place")
    out, _ = run_project(G, sel, ld, n, g, v32, inplace=inplace, **kw)
    ulps = ulp_distance(torch.from_numpy(out), torch.from_numpy(want))
    print("MEASURED|%s|project %s ulp|%d|0" % (case, what, ulps))
    assert np_bits_equal(out, want), "project %s: %d ulp from the float64 loop rounded once" % (what, ulps)
    # the device-coefficient form: v as f64, rounded to float32 by the kernel
    outd, _ = run_project(G, sel, ld, n, g, v64, info=(2, 0), inplace=inplace, **kw)
    ulps = ulp_distance(torch.from_numpy(outd), torch.from_numpy(want))
    print("MEASURED|%s|project_dev %s ulp|%d|0" % (case, what, ulps))
    assert np_bits_equal(outd, want), "project_dev %s: %d ulp from the float64 loop on float32(v)" % (what, ulps)
    assert np_bits_equal(outd, out), "project_dev differs from project given float32(v)"
    # nothing violated: the gradient stays as it is
    out0, g0 = run_project(G, sel, ld, n, g, v64, info=(0, 0), inplace=inplace, **kw)
    assert np_bits_equal(g0, g), "info[0] = 0: g changed"
    assert np_bits_equal(out0, g), "info[0] = 0: out is not g bit for bit"


@pytest.mark.parametrize("path", list(PROJ_PATHS))
@pytest.mark.parametrize("m", [1, 3, 11, 16])
def test_project_and_project_dev(request, m, path):
    for n in (1, 3, 4, 5, 1027):
        for inplace in (False, True):
            check_project(request.node.name, m, n, path, inplace)


@pytest.mark.parametrize("path", list(PROJ_PATHS))
def test_project_second_stride_trip(request, path):
    """n > 2048 * 256 * 4: the 16-byte loop's second trip (the scalar loop's fifth), ragged end."""
    assert BIG_PROJ // 4 > CAP * GB and BIG_PROJ % 4 == 3
    check_project(request.node.name, 3, BIG_PROJ, path, False)
    check_project(request.node.name, 3, BIG_PROJ, path, True)


@pytest.mark.parametrize("path", ["aligned", "ld%4"])
@pytest.mark.parametrize("m", [1, 3, 16])
def test_project_dev_unviolated_ignores_the_memory(request, m, path):
    """info[0] == 0 and out != g: out is g bit for bit even when a memory row holds Inf / NaN inside n (gem.py:275-277 leaves
    the gradient alone; g + 0.0 * G[row] would give NaN there).  Failed before project_dev_kernel skipped the row loop:
    every poisoned column of out came back NaN (m = 1, 3, 16, both paths)."""
    kw = PROJ_PATHS[path]
    for n in (5, 1027):
        G, sel, ld, g, v64 = proj_data(m, n, bool(kw.get("ld_odd")))
        G = G.copy()
        G[sel[0], 0] = np.inf
        G[sel[-1], n - 1] = np.nan
        G[sel[m // 2], n // 2] = -np.inf
        out, g_after = run_project(G, sel, ld, n, g, v64, info=(0, 0), **kw)
        print("MEASURED|%s|unviolated m=%d n=%d non-finite out|%d|0" % (request.node.name, m, n, int((~np.isfinite(out)).sum())))
        assert np_bits_equal(out, g) and np_bits_equal(g_after, g), "out != g although nothing is violated"
        # violated: the poison does propagate, to exactly its columns
        out, _ = run_project(G, sel, ld, n, g, v64, info=(1, 0), **kw)
        bad = sorted({0, n - 1, n // 2})
        assert sorted(np.nonzero(~np.isfinite(out))[0].tolist()) == bad


# ===================================================================================================== the chain
def chain_problem(kind, t, n):
    """Memory rows M[t][n] and the gradient g on the grid k / 16, |k| <= 24: every Gram entry is then an exact float64 in any
    summation order, so the device solves the QP of exactly the matrix the host reference sees."""
    rs = np.random.RandomState(100 * t + len(kind))
    M = rs.randint(-8, 9, size=(t, n)).astype(np.float32) / 8
    g = rs.randint(-8, 9, size=n).astype(np.float32) / 8
    margin = 0.0
    if kind == "all-violated":
        c = rs.randint(-8, 9, size=n).astype(np.float32) / 8
        M = M / 2 + c
        g = -c
    elif kind == "identical-rows":
        M[t // 2] = M[0]
        g = -(M[0] + M[-1]) / 2 + g / 4
    else:
        margin = 0.5
        g = g / 4 - 2 * M[0] - M[t - 1]                    # two strongly violated constraints: their v lie above the margin
    return M, g, margin


@pytest.mark.parametrize("t", [15, 4])
@pytest.mark.parametrize("kind", ["all-violated", "identical-rows", "margin-boundary"])
def test_chain_gram_qp_project(request, kind, t):
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
    if kind == "all-violated":
        assert viol == t
    elif kind == "identical-rows":
        assert viol > 0 and np.array_equal(gram64[0], gram64[t // 2])
    else:
        assert viol > 0 and int((np.abs(v_host - margin) <= 1e-9).sum()) >= 1 and int((v_host > margin + 1e-3).sum()) >= 1, v_host
    ar = Arena()
    kG = ar.add(torch.from_numpy(G))
    ko = ar.add(n, fill=OUT_BITS)
    ar.upload(dev())
    need = L.clhip_gem_gram_ws(m)
    ws = Guarded(torch.float64, need // 8, fill_bits=NAN64_BITS)
    gram = Guarded(torch.float64, m * m, fill_bits=NAN64_BITS)
    v = Guarded(torch.float64, t, fill_bits=NAN64_BITS)
    info = Guarded(torch.int32, 2, fill_bits=-1)
    s = stream()
    g_ptr = ar.ptr(kG) + 4 * (t + 1) * ld
    assert L.clhip_gem_gram(ar.ptr(kG), ld, (C.c_int * m)(*sel), m, n, gram.ptr, ws.ptr, need, s) == 0
    assert L.clhip_gem_qp(gram.ptr, m, C.c_double(margin), C.c_double(1e-3), v.ptr, info.ptr, s) == 0
    assert L.clhip_gem_project_dev(ar.ptr(kG), ld, (C.c_int * t)(*order), v.ptr, info.ptr, t, g_ptr, ar.ptr(ko), n, s) == 0
    torch.cuda.synchronize()                              # the only host contact of the chain
    ar.download()
    assert ar.gaps_untouched() and bitwise_equal(ar.get(kG), torch.from_numpy(G).reshape(-1))
    gram_dev = gram.get()[0].numpy().reshape(m, m)
    bound = np.maximum(n * 2.0 ** -53 * terms, np.finfo(np.float64).tiny)
    r_gram = float((np.abs(gram_dev.astype(np.longdouble) - ref) / bound).max())
    v_dev = v.get()[0].numpy().copy()
    assert info.get()[0].tolist() == [viol, 0]
    scale = max(1.0, float(np.abs(v_host).max()))
    r_v = float(np.abs(v_dev - v_host).max()) / (1e-9 * scale)
    print("MEASURED|%s|gram|%.3e|0" % (request.node.name, r_gram))
    print("MEASURED|%s|v (max |v| %.3g)|%.3e|0" % (request.node.name, scale, r_v))
    assert r_gram <= 1.0 and r_v <= 1.0, (r_gram, r_v)
    want = project_reference(G, order, n, g, v_dev.astype(np.float32))
    out = ar.get(ko).numpy()
    ulps = ulp_distance(torch.from_numpy(out.copy()), torch.from_numpy(want))
    print("MEASURED|%s|projected gradient ulp|%d|0" % (request.node.name, ulps))
    assert np_bits_equal(out, want), "%d ulp from the float64 loop on the device's own float32(v)" % ulps
    assert float(np.abs(v_dev).max()) > 0 and not np_bits_equal(out, g)
