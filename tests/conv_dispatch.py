"""The launch decisions of csrc/conv2d.hip, csrc/convkk.hip, the 5x5 entry points of csrc/bsconv.hip and csrc/bswgrad5.hip restated
in Python (test infrastructure shared by test_gpu_conv2d_kernels.py, test_gpu_conv5x5_bs_kernels.py and test_conv_args_cpu.py).
Nothing here calls the library; the tests compare what the library does with these rules.

The three products of a convolution layer as the gather-GEMM  C[M][Nn] = sum_kd A(m, kd) B(kd, n)  of conv2d_gemm_kernel<OP, RT, CT>
(a block owns 64 RT rows x 64 CT columns):
  fwd          y  : (M, Nn, Kd) = (K, N*OH*OW, C*R*S)
  bwd_data     dx : (M, Nn, Kd) = (C, N*H*W,   K*R*S)
  bwd_weight   dw : (M, Nn, Kd) = (K, C*R*S,   N*OH*OW), split over Kd into `splits` slabs of k_per_split (a multiple of 32)
Forward and backward-data of a 5x5 / stride 1 / pad 2 layer go to convkk_kernel<5, MODE> (the "halo" kernel) where
clhip_internal_convkk_ok allows it."""
from collections import namedtuple

TM = TN = 64
BK = 32
TAB_MAX = 256
BIAS_SPLIT = 16
MAX_ELEMS = 0x1fffffff
KINDS = ("fwd", "bwd_data", "bwd_weight")

# kernel "gemm": rt, ct = the template arguments, m_tiles x n_tiles blocks per split; kernel "halo": rt = ct = 0,
# m_tiles = 64-channel groups, n_tiles = N * (384-pixel parts of a plane), splits = 1.
# w_inc: the weight gradient steps (img, oh, ow) with carries (True) or decodes them with divisions (False, tiny planes);
# empty: the last split(s) begin behind Kd and only write zeros.  Both are None where they do not apply.
Plan = namedtuple("Plan", "kernel rt ct m_tiles n_tiles splits w_inc empty")


# ------------------------------------------------------------------------------------------------ conv2d.hip
def conv_ok(N, C, H, W, K, R, S, st, pad):
    """(OH, OW), or None where every clhip_conv2d_* call answers CLHIP_EINVAL (and clhip_conv2d_bwd_weight_ws 0)."""
    if N <= 0 or C <= 0 or H <= 0 or W <= 0 or K <= 0 or R <= 0 or S <= 0 or st <= 0 or pad < 0:
        return None
    if R > 255 or S > 255:
        return None
    OH, OW = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    if H + 2 * pad - R < 0 or W + 2 * pad - S < 0 or OH <= 0 or OW <= 0:
        return None
    if N * C * H * W > MAX_ELEMS or N * K * OH * OW > MAX_ELEMS:
        return None
    return OH, OW


def row_tiles(M):
    """The tile height (in units of 64 rows) that pads M least, the larger on ties."""
    best, best_pad = 1, -1
    for rt in (1, 2, 3):
        pad = (M + 64 * rt - 1) // (64 * rt) * 64 * rt
        if best_pad < 0 or pad <= best_pad:
            best, best_pad = rt, pad
    return best


def col_tiles(M, Nn, wgrad=False):
    return 2 if (row_tiles(M) >= 2 or not wgrad) and Nn > 64 else 1


def tile_counts(M, Nn, wgrad=False):
    rt, ct = row_tiles(M), col_tiles(M, Nn, wgrad)
    return (M + TM * rt - 1) // (TM * rt), (Nn + TN * ct - 1) // (TN * ct)


def wgrad_splits(M, Nn, Kd):
    rt, ct = row_tiles(M), col_tiles(M, Nn, True)
    mt, nt = tile_counts(M, Nn, True)
    s = (512 if rt * ct > 1 else 1024) // (mt * nt)
    return max(1, min(s, Kd // 256, 256))


def k_per_split(Kd, splits):
    return ((Kd + splits - 1) // splits + BK - 1) // BK * BK


def live_splits(Kd, splits):
    kps = k_per_split(Kd, splits)
    return (Kd + kps - 1) // kps


def gemm_dims(kind, shape):
    N, C, H, W, K, R, S, st, pad = shape
    OH, OW = conv_ok(*shape)
    if kind == "fwd":
        return K, N * OH * OW, C * R * S
    if kind == "bwd_data":
        return C, N * H * W, K * R * S
    assert kind == "bwd_weight"
    return K, C * R * S, N * OH * OW


def bwd_weight_ws_bytes(shape):
    if conv_ok(*shape) is None:
        return 0
    N, C, H, W, K, R, S, st, pad = shape
    M, Nn, Kd = gemm_dims("bwd_weight", shape)
    return max(4 * K * C * R * S * wgrad_splits(M, Nn, Kd), 8 * K * BIAS_SPLIT)


# ------------------------------------------------------------------------------------------------ convkk.hip
QKT, QCK, QPW, QROWS, QPIX = 64, 4, 32, 20, 384


def convkk_rows(H, W, pad):
    HW = H * W
    worst = 0
    for part in range((HW + QPIX - 1) // QPIX):
        p0 = part * QPIX
        p1 = min(p0 + QPIX - 1, HW - 1)
        worst = max(worst, p1 // W - p0 // W + 1 + 2 * pad)
    return worst


def convkk_ok(N, Cin, Cout, H, W, R, S, st, pad):
    """Cin / Cout as the KERNEL sees them: (C, K) forward, (K, C) backward-data."""
    if R != 5 or S != 5 or st != 1 or pad != 2:
        return False
    if N <= 0 or Cin % QCK or Cin < QCK or Cout % 32 or H < 1 or W < 1 or W + 2 * pad > QPW:
        return False
    if convkk_rows(H, W, pad) > QROWS:
        return False
    return N * Cin * H * W * 4 < 1 << 31 and N * Cout * H * W * 4 < 1 << 31 and Cin * Cout * R * S * 4 < 1 << 31


def halo_refusal(N, Cin, Cout, H, W, R, S, st, pad):
    """Why convkk_ok turns a 5x5 / 1 / 2 shape down: 'channels', 'width', 'rows' or None."""
    assert (R, S, st, pad) == (5, 5, 1, 2)
    if Cin % QCK or Cin < QCK or Cout % 32:
        return "channels"
    if W + 2 * pad > QPW:
        return "width"
    if convkk_rows(H, W, pad) > QROWS:
        return "rows"
    return None


def plan(kind, shape, halo=True):
    """What the entry point of `kind` launches for `shape` (halo=False: a library built with CLHIP_NO_HALO_CONV)."""
    N, C, H, W, K, R, S, st, pad = shape
    OH, OW = conv_ok(*shape)
    if halo and kind == "fwd" and convkk_ok(N, C, K, H, W, R, S, st, pad):
        return Plan("halo", 0, 0, (K + QKT - 1) // QKT, N * ((H * W + QPIX - 1) // QPIX), 1, None, None)
    if halo and kind == "bwd_data" and convkk_ok(N, K, C, H, W, R, S, st, pad):
        return Plan("halo", 0, 0, (C + QKT - 1) // QKT, N * ((H * W + QPIX - 1) // QPIX), 1, None, None)
    M, Nn, Kd = gemm_dims(kind, shape)
    wg = kind == "bwd_weight"
    mt, nt = tile_counts(M, Nn, wg)
    if not wg:
        return Plan("gemm", row_tiles(M), col_tiles(M, Nn), mt, nt, 1, None, None)
    splits = wgrad_splits(M, Nn, Kd)
    return Plan("gemm", row_tiles(M), col_tiles(M, Nn, True), mt, nt, splits, BK // OW + 1 <= OH, live_splits(Kd, splits) < splits)


# ------------------------------------------------------------------------------------------------ bsconv.hip, 5x5
BS_BN, BS_CK = 64, 16


def bs_ok(Cin, Cout, H, W):
    return Cin >= 32 and Cin % 32 == 0 and Cout % 64 == 0 and H >= 4 and W >= 4


def bs5_ok(kind, N, C, K, H, W):
    """clhip_conv5x5_bs_fwd / _bwd_data take the shape (CLHIP_ENOTSUP otherwise); the kernel's (Cin, Cout) is (C, K) / (K, C)."""
    cin, cout = (C, K) if kind == "fwd" else (K, C)
    return N > 0 and bs_ok(cin, cout, H, W) and W > 8


def bs5_geometry(H, W):
    """(RW, RH) of the block: BsGeo<16,8,..,5> up to 16 columns, BsGeo<32,4,..,5> above."""
    return (32, 4) if W > 16 else (16, 8)


def bs5_epilogue(H, W):
    """How bs_conv_body stores its tile: odd maps lane by lane ("scalar"); even maps with W % 4 == 0 as whole float4 row pieces
    through LDS ("float4", the mask of backward-data loaded as float4 too); other even maps as float2 window rows ("float2")."""
    if (H | W) & 1:
        return "scalar"
    return "float4" if W % 4 == 0 else "float2"


def bs5_blocks(N, Cout, H, W):
    """(pixel blocks npb, blocks launched): pixel blocks are dealt out in groups of 8, one per XCD; the grid is padded to whole groups."""
    rw, rh = bs5_geometry(H, W)
    npb = ((W + rw - 1) // rw) * ((H + rh - 1) // rh) * N
    return npb, (npb + 7) // 8 * 8 * ((Cout + BS_BN - 1) // BS_BN)


def bs5_image_bytes(Cin, Cout):
    """clhip_internal_bs5_ws: the weight image one call writes."""
    return ((Cout + 31) // 32) * ((Cin + BS_CK - 1) // BS_CK) * 75 * 1024


def bs5_ws_bytes(C, K):
    """clhip_conv5x5_bs_ws: one workspace for forward and backward-data of a layer."""
    return max(bs5_image_bytes(C, K), bs5_image_bytes(K, C))


# ------------------------------------------------------------------------------------------------ bswgrad5.hip, KS = 5
def bsk5_ok(N, C, K, H, W):
    return N >= 1 and C >= 32 and C % 32 == 0 and K >= 32 and K % 32 == 0 and W >= 8 and H >= 1 and \
        N * C * H * W * 4 < 0x7fffffff and N * K * H * W * 4 < 0x7fffffff


def bsk5_splits(N, C, K, H, W):
    types = (K // 32) * (C // 32) * 5
    rows = N * ((W + 15) // 16) * H
    return max(1, min(2048 // types, rows))


def bsk5_ws_bytes(N, C, K, H, W):
    return bsk5_splits(N, C, K, H, W) * (25 * K * C + K) * 4 if bsk5_ok(N, C, K, H, W) else 0


# ------------------------------------------------------------------------------------------------ the cases
G, HALO = "gemm", "halo"


def _g(rt, ct, mt, nt, splits=1, w_inc=None, empty=None):
    return Plan(G, rt, ct, mt, nt, splits, w_inc, empty)


def _h(kts, blocks):
    return Plan(HALO, 0, 0, kts, blocks, 1, None, None)


# (N, C, H, W, K, R, S, stride, pad), what the row is there for, the launch of each entry point — worked out by hand from the
# conditions of conv2d.hip and convkk.hip; check_case_table() asserts that plan() reproduces every row.
CASES = [
    ((1, 5, 6, 6, 40, 3, 3, 1, 1), "all tiles ragged",
     {"fwd": _g(1, 1, 1, 1), "bwd_data": _g(1, 1, 1, 1), "bwd_weight": _g(1, 1, 1, 1, 1, True, False)}),
    ((1, 3, 9, 9, 72, 3, 3, 1, 0), "",
     {"fwd": _g(2, 1, 1, 1), "bwd_data": _g(1, 2, 1, 1), "bwd_weight": _g(2, 1, 1, 1, 1, True, False)}),
    ((1, 72, 7, 7, 72, 3, 3, 1, 1), "",
     {"fwd": _g(2, 1, 1, 1), "bwd_data": _g(2, 1, 1, 1), "bwd_weight": _g(2, 2, 1, 6, 1, True, False)}),
    ((2, 72, 9, 9, 72, 3, 5, 1, 1), "R != S",
     {"fwd": _g(2, 2, 1, 1), "bwd_data": _g(2, 2, 1, 2), "bwd_weight": _g(2, 2, 1, 9, 1, True, False)}),
    ((1, 3, 8, 8, 130, 3, 3, 1, 0), "",
     {"fwd": _g(3, 1, 1, 1), "bwd_data": _g(1, 1, 1, 1), "bwd_weight": _g(3, 1, 1, 1, 1, True, False)}),
    ((1, 130, 6, 6, 130, 3, 3, 1, 1), "",
     {"fwd": _g(3, 1, 1, 1), "bwd_data": _g(3, 1, 1, 1), "bwd_weight": _g(3, 2, 1, 10, 1, True, False)}),
    ((2, 130, 9, 11, 130, 5, 3, 2, 2), "R != S, stride 2, H != W",
     {"fwd": _g(3, 2, 1, 1), "bwd_data": _g(3, 2, 1, 2), "bwd_weight": _g(3, 2, 1, 16, 1, True, False)}),
    ((1, 2, 26, 26, 200, 3, 3, 1, 0), "bwd_weight: 2 row tiles x 2 splits",
     {"fwd": _g(2, 2, 2, 5), "bwd_data": _g(1, 2, 1, 6), "bwd_weight": _g(2, 1, 2, 1, 2, True, False)}),
    ((16, 2, 9, 25, 8, 3, 3, 1, 0), "bwd_weight: 10 splits, the last one empty (k_begin = 2592 > Kd = 2576)",
     {"fwd": _g(1, 2, 1, 21), "bwd_data": _g(1, 2, 1, 29), "bwd_weight": _g(1, 1, 1, 1, 10, True, True)}),
    ((2, 4, 12, 9, 20, 7, 2, 3, 1), "R != S, stride 3 > S (dx columns no window touches), w_inc false",
     {"fwd": _g(1, 1, 1, 1), "bwd_data": _g(1, 2, 1, 2), "bwd_weight": _g(1, 1, 1, 1, 1, False, False)}),
    ((3, 3, 35, 35, 64, 11, 11, 4, 2), "AlexNet conv1 geometry, 35 -> 8",
     {"fwd": _g(1, 2, 1, 2), "bwd_data": _g(1, 2, 1, 29), "bwd_weight": _g(1, 1, 1, 6, 1, True, False)}),
    ((1, 3, 5, 5, 8, 2, 2, 1, 3), "pad 3 >= R = S = 2: windows that lie entirely in the padding",
     {"fwd": _g(1, 2, 1, 1), "bwd_data": _g(1, 1, 1, 1), "bwd_weight": _g(1, 1, 1, 1, 1, True, False)}),
    ((100, 4, 4, 5, 8, 3, 3, 1, 0), "bwd_weight: OH = 2, OW = 3 (w_inc false) with 2 splits",
     {"fwd": _g(1, 2, 1, 5), "bwd_data": _g(1, 2, 1, 16), "bwd_weight": _g(1, 1, 1, 1, 2, False, False)}),
    ((1, 3, 7, 7, 8, 2, 2, 3, 0), "stride 3 > R = S = 2: dx rows and columns no window touches",
     {"fwd": _g(1, 1, 1, 1), "bwd_data": _g(1, 1, 1, 1), "bwd_weight": _g(1, 1, 1, 1, 1, False, False)}),
    # 5x5 / stride 1 / pad 2: the halo kernel
    ((2, 32, 13, 28, 96, 5, 5, 1, 2), "fwd Cout = 96; bwd_data Cout = 32 (the ka break); W + 4 == 32; one part with idle slots",
     {"fwd": _h(2, 2), "bwd_data": _h(1, 2), "bwd_weight": _g(2, 2, 1, 7, 2, True, False)}),
    ((1, 96, 20, 28, 32, 5, 5, 1, 2), "fwd Cout = 32; bwd_data Cout = 96; two parts, the second from row 13, column 20",
     {"fwd": _h(1, 2), "bwd_data": _h(2, 2), "bwd_weight": _g(1, 1, 1, 38, 2, True, False)}),
    ((2, 64, 27, 27, 32, 5, 5, 1, 2), "AlexNet's map, two parts",
     {"fwd": _h(1, 4), "bwd_data": _h(1, 4), "bwd_weight": _g(1, 1, 1, 25, 5, True, False)}),
    # 5x5 / 1 / 2 shapes convkk_ok refuses: they must land on the gather-GEMM
    ((2, 30, 13, 28, 96, 5, 5, 1, 2), "halo refused for channels (C = 30: fwd Cin % 4, bwd_data Cout % 32)",
     {"fwd": _g(2, 2, 1, 6), "bwd_data": _g(1, 2, 1, 6), "bwd_weight": _g(2, 2, 1, 6, 2, True, False)}),
    ((1, 32, 6, 29, 32, 5, 5, 1, 2), "halo refused for width (W + 4 = 33)",
     {"fwd": _g(1, 2, 1, 2), "bwd_data": _g(1, 2, 1, 2), "bwd_weight": _g(1, 1, 1, 13, 1, True, False)}),
    ((1, 32, 30, 16, 32, 5, 5, 1, 2), "halo refused for rows (384 pixels = 24 rows + 4 > 20)",
     {"fwd": _g(1, 2, 1, 4), "bwd_data": _g(1, 2, 1, 4), "bwd_weight": _g(1, 1, 1, 13, 1, True, False)}),
]
HALO_REFUSED = {(2, 30, 13, 28, 96, 5, 5, 1, 2): "channels", (1, 32, 6, 29, 32, 5, 5, 1, 2): "width", (1, 32, 30, 16, 32, 5, 5, 1, 2): "rows"}

# The eighteen instantiations conv2d.hip builds minus <WGRAD,1,2>: col_tiles(M, Nn, wgrad=True) is 2 only when row_tiles(M) >= 2
# (one row tile next to two column tiles lost on AlexNet's conv1 weight gradient), so no call can select it.
REACHABLE = {(kind, rt, ct) for kind in KINDS for rt in (1, 2, 3) for ct in (1, 2)} - {("bwd_weight", 1, 2)}


def halo_cases():
    return [(s, k) for s, _, row in CASES for k in ("fwd", "bwd_data") if row[k].kernel == HALO]


def check_case_table():
    seen = set()
    for shape, note, row in CASES:
        assert conv_ok(*shape) is not None, shape
        for kind in KINDS:
            p = plan(kind, shape)
            assert p == row[kind], (shape, kind, p, row[kind])
            if p.kernel == G:
                seen.add((kind, p.rt, p.ct))
            nh = plan(kind, shape, halo=False)
            assert nh.kernel == G and (p.kernel == HALO or nh == p)
        N, C, H, W, K, R, S, st, pad = shape
        if (R, S, st, pad) == (5, 5, 1, 2):
            why_f, why_d = halo_refusal(N, C, K, H, W, R, S, st, pad), halo_refusal(N, K, C, H, W, R, S, st, pad)
            assert (why_f is None) == (row["fwd"].kernel == HALO) and (why_d is None) == (row["bwd_data"].kernel == HALO)
            if shape in HALO_REFUSED:
                assert why_f == why_d == HALO_REFUSED[shape], (shape, why_f, why_d)
        else:
            assert not convkk_ok(N, C, K, H, W, R, S, st, pad) and not convkk_ok(N, K, C, H, W, R, S, st, pad)
    assert len(REACHABLE) == 17 and seen == REACHABLE, sorted(REACHABLE - seen)
    assert sorted(HALO_REFUSED.values()) == ["channels", "rows", "width"] and all(s in [c[0] for c in CASES] for s in HALO_REFUSED)
    for M in range(1, 1025):                       # <WGRAD,1,2> really is unreachable: no M with row_tiles 1 gets two column tiles
        assert not (row_tiles(M) == 1 and col_tiles(M, 10 ** 6, True) == 2)
    flags = [(row["bwd_weight"].splits > 1, row["bwd_weight"].w_inc, row["bwd_weight"].empty, row["bwd_weight"].m_tiles > 1) for _, _, row in CASES]
    assert any(sp and mt for sp, wi, em, mt in flags), "more than one row tile together with more than one split"
    assert any(em for sp, wi, em, mt in flags), "an empty last split"
    assert any(sp and not wi for sp, wi, em, mt in flags), "the division decode together with more than one split"
    assert any(s[5] != s[6] for s, _, _ in CASES) and any(s[8] >= s[5] for s, _, _ in CASES) and any(s[7] > max(s[5], s[6]) for s, _, _ in CASES)


# bf16-split 5x5 forward / backward-data: (N, C, K, H, W), which entry points take it, (RW, RH), what it covers
BS5_CASES = [
    ((1, 32, 64, 4, 9), ("fwd",), (16, 8), "both minima; backward-data refuses (32 output channels)"),
    ((2, 64, 64, 9, 16), ("fwd", "bwd_data"), (16, 8), "last row tile has one row; W at the switch"),
    ((1, 64, 128, 5, 17), ("fwd", "bwd_data"), (32, 4), "one-row tail, 15 idle columns, two channel groups"),
    ((1, 96, 64, 4, 33), ("fwd",), (32, 4), "six chunks; the second column tile has one column"),
    ((3, 64, 96, 7, 27), ("bwd_data",), (32, 4), "AlexNet's width; forward refuses (96 output channels)"),
    ((9, 64, 64, 4, 9), ("fwd", "bwd_data"), (16, 8), "nine pixel blocks cross the 8-block XCD group"),
    # even maps: the epilogues that store vectors (every row above has an odd H or W and stores scalars)
    ((2, 64, 64, 8, 20), ("fwd", "bwd_data"), (32, 4), "float4 row stores and float4 mask loads, 12 idle columns"),
    ((1, 64, 64, 4, 12), ("fwd", "bwd_data"), (16, 8), "float4 row stores in the 16-wide geometry, half the rows idle"),
    ((1, 64, 64, 6, 18), ("fwd", "bwd_data"), (32, 4), "W % 4 == 2: float2 window stores and float2 mask loads"),
]
# bf16-split 5x5 weight gradient: (N, C, K, H, W), splits, what it covers
BSK5_CASES = [
    ((1, 32, 32, 1, 8), 1, "minimum W: every half == 1 lane has nd == 0"),
    ((2, 32, 64, 3, 9), 6, ""),
    ((1, 64, 32, 6, 27), 12, ""),
    ((3, 32, 32, 2, 33), 18, "three strips; the last has one column"),
    ((2, 64, 64, 27, 27), 102, "102 shares over 108 rows: shares straddle strips and images"),
]


def check_bs_tables():
    for (N, C, K, H, W), kinds, geo, _ in BS5_CASES:
        assert bs5_geometry(H, W) == geo
        for kind in ("fwd", "bwd_data"):
            assert bs5_ok(kind, N, C, K, H, W) == (kind in kinds), ((N, C, K, H, W), kind)
    assert bs5_blocks(9, 64, 4, 9) == (9, 16) and bs5_blocks(2, 64, 9, 16) == (4, 8)
    assert {bs5_epilogue(s[3], s[4]) for s, _, _, _ in BS5_CASES} == {"scalar", "float4", "float2"}
    assert {(bs5_geometry(s[3], s[4]), bs5_epilogue(s[3], s[4])) for s, _, _, _ in BS5_CASES} >= {((32, 4), "float4"), ((16, 8), "float4")}
    for (N, C, K, H, W), splits, _ in BSK5_CASES:
        assert bsk5_ok(N, C, K, H, W) and bsk5_splits(N, C, K, H, W) == splits, ((N, C, K, H, W), bsk5_splits(N, C, K, H, W))
