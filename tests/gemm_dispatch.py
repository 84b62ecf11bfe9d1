"""The launch decisions of csrc/gemm.hip restated in Python (test infrastructure shared by test_gpu_gemm_kernels.py and
test_gemm_args_cpu.py): wide_ok, choose_splits, choose_splits_wide, k_per_split, the number of live splits and the bytes of
workspace one call needs.  Nothing here calls the library; the tests compare what the library does with these rules.

A Linear layer's three products as the strided GEMM  C[M][N] = sum_k A(m,k) B(k,n)  of gemm_launch<AK, BKc>:
  fwd          y  = x . w^T    (M, N, K) = (batch, O, I)   A = x  (k contiguous), B(k,n) = w[n][k]  (k contiguous)   <1,1>
  bwd_data     dx = dy . w     (M, N, K) = (batch, I, O)   A = dy (k contiguous), B(k,n) = w[k][n]  (n contiguous)   <1,0>
  bwd_weight   dw = dy^T . x   (M, N, K) = (O, I, batch)   A(m,k) = dy[k][m] (m contiguous), B(k,n) = x[k][n]        <0,0>
"""
from collections import namedtuple

TM = 64          # gemm_mfma_kernel: 64 x 64 output tile
WT = 128         # gemm_wide_kernel: 128 x 128 output tile
BK = 32          # depth of a staged k chunk; k_per_split is a multiple of it
KINDS = ("fwd", "bwd_data", "bwd_weight")

Gemm = namedtuple("Gemm", "M N K AK BKc sam sak sbk sbn")
Plan = namedtuple("Plan", "tile splits k_per_split live tail need_bytes")


def fc_gemm(kind, M, I, O):
    """(batch M, in I, out O) of a Linear layer -> the GEMM its entry point launches."""
    if kind == "fwd":
        return Gemm(M, O, I, True, True, I, 1, 1, I)
    if kind == "bwd_data":
        return Gemm(M, I, O, True, False, O, 1, I, 1)
    assert kind == "bwd_weight"
    return Gemm(O, I, M, False, False, 1, O, I, 1)


def wide_ok(g, a_aligned=True, b_aligned=True):
    if g.M < WT or g.N < 8 * WT or (g.K & 3):
        return False
    if not (a_aligned and b_aligned):
        return False
    if (g.sam & 3) if g.AK else ((g.sak & 3) or (g.M & 3)):
        return False
    if (g.sbn & 3) if g.BKc else ((g.sbk & 3) or (g.N & 3)):
        return False
    return True


def _splits(M, N, K, T, min_k):
    tiles = ((M + T - 1) // T) * ((N + T - 1) // T)
    return max(1, min(512 // tiles, K // min_k, 32))


def choose_splits(M, N, K):
    return _splits(M, N, K, TM, 96)


def choose_splits_wide(M, N, K):
    return _splits(M, N, K, WT, 128)


def plan(g, a_aligned=True, b_aligned=True, ws_bytes=None):
    """What gemm_launch does with this problem.  ws_bytes=None: a workspace of any size the call may want; 0: no workspace.
    need_bytes is what the call wants before the fallback to one split (0 when it wants none)."""
    wide = wide_ok(g, a_aligned, b_aligned)
    splits = choose_splits_wide(g.M, g.N, g.K) if wide else choose_splits(g.M, g.N, g.K)
    need = 4 * g.M * g.N * splits if splits > 1 else 0
    if splits > 1 and ws_bytes is not None and ws_bytes < need:
        splits = 1
    kps = ((g.K + splits - 1) // splits + BK - 1) // BK * BK
    live = (g.K + kps - 1) // kps
    return Plan("wide" if wide else "64", splits, kps, live, g.K - (live - 1) * kps, need)


def fc_plan(kind, M, I, O, **kw):
    return plan(fc_gemm(kind, M, I, O), **kw)


def fc_ws_bytes(M, I, O):
    """clhip_fc_ws: one workspace for the three calls of a layer, whichever tile kernel each of them gets."""
    if M <= 0 or I <= 0 or O <= 0:
        return 0

    def sp(m, n, k):
        return max(choose_splits(m, n, k), choose_splits_wide(m, n, k))
    return 4 * max(M * O * sp(M, O, I), M * I * sp(M, I, O), O * I * sp(O, I, M))


# (M, I, O) -> per kind (tile kernel, splits launched, live splits, depth of the last live split), worked out by hand from
# the conditions of gemm.hip; both test files assert that fc_plan() reproduces every row.
CASES = [
    ((1, 1, 1),         {"fwd": ("64", 1, 1, 1),       "bwd_data": ("64", 1, 1, 1),     "bwd_weight": ("64", 1, 1, 1)}),
    ((7, 50, 33),       {"fwd": ("64", 1, 1, 50),      "bwd_data": ("64", 1, 1, 33),    "bwd_weight": ("64", 1, 1, 7)}),
    ((33, 97, 31),      {"fwd": ("64", 1, 1, 97),      "bwd_data": ("64", 1, 1, 31),    "bwd_weight": ("64", 1, 1, 33)}),
    ((65, 500, 65),     {"fwd": ("64", 5, 4, 116),     "bwd_data": ("64", 1, 1, 65),    "bwd_weight": ("64", 1, 1, 65)}),
    ((3, 500, 5),       {"fwd": ("64", 5, 4, 116),     "bwd_data": ("64", 1, 1, 5),     "bwd_weight": ("64", 1, 1, 3)}),
    ((5, 3000, 7),      {"fwd": ("64", 31, 24, 56),    "bwd_data": ("64", 1, 1, 7),     "bwd_weight": ("64", 1, 1, 5)}),
    ((64, 3104, 64),    {"fwd": ("64", 32, 25, 32),    "bwd_data": ("64", 1, 1, 64),    "bwd_weight": ("64", 1, 1, 64)}),
    ((200, 128, 20),    {"fwd": ("64", 1, 1, 128),     "bwd_data": ("64", 1, 1, 20),    "bwd_weight": ("64", 2, 2, 72)}),
    ((130, 36, 1027),   {"fwd": ("wide", 1, 1, 36),    "bwd_data": ("64", 10, 9, 3),    "bwd_weight": ("64", 1, 1, 130)}),
    ((129, 324, 1025),  {"fwd": ("wide", 2, 2, 132),   "bwd_data": ("64", 10, 9, 1),    "bwd_weight": ("64", 1, 1, 129)}),
    ((132, 388, 1028),  {"fwd": ("wide", 3, 3, 68),    "bwd_data": ("64", 10, 9, 4),    "bwd_weight": ("64", 1, 1, 132)}),
    ((130, 1028, 132),  {"fwd": ("64", 10, 9, 4),      "bwd_data": ("wide", 1, 1, 132), "bwd_weight": ("64", 1, 1, 130)}),
    ((132, 1028, 260),  {"fwd": ("64", 10, 9, 4),      "bwd_data": ("wide", 2, 2, 100), "bwd_weight": ("wide", 1, 1, 132)}),
    ((260, 1024, 128),  {"fwd": ("64", 10, 8, 128),    "bwd_data": ("wide", 1, 1, 128), "bwd_weight": ("wide", 2, 2, 100)}),
    ((128, 1024, 4),    {"fwd": ("64", 10, 8, 128),    "bwd_data": ("wide", 1, 1, 4),   "bwd_weight": ("64", 1, 1, 128)}),
]


def check_case_table():
    for (M, I, O), row in CASES:
        for kind in KINDS:
            p = fc_plan(kind, M, I, O)
            assert (p.tile, p.splits, p.live, p.tail) == row[kind], ((M, I, O), kind, p, row[kind])
