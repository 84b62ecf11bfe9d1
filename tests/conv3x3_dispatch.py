"""The launch decisions of csrc/conv3x3.hip and csrc/conv3x3_wgrad.hip restated in Python (test infrastructure shared by
test_conv3x3_args_cpu.py and test_gpu_conv3x3_kernels.py).  Nothing here calls the library; the tests compare what the library does
with these rules.

Forward and backward-data run the SAME chunked kernels (conv3x3_mfma_kernel / _mixed_kernel / _mixed2_kernel): the kernel's
(Cin, Cout) is the layer's (C, K) forward and (K, C) backward-data.  Forward stages CK = 4 channels per chunk for C <= 4 and 8
otherwise; backward-data always 8.

dims_ok.  What the kernels' 32-bit index arithmetic carries, read from the code: the chunked body forms BYTE offsets in int relative
to the first image of its tile group (`in_blk`, at most NB = 2 images): ((nb Cin + cl) H W + h W + w) * 4 + c0 H W * 4 < 2 Cin H W * 4,
the same for the output / mask_src with Cout, and (k Cw 9 + ...) * 4 < 9 K C * 4 for the weights; the weight gradient's staging forms
(cl H W + ...) * 4 for cl < 64 whatever C is; launch_geo multiplies tiles_w * tiles_h * ngrp <= N H W in int.  The first-layer
kernels index in size_t or have limits of their own (c3w64_shape: 2^29 elements of x and of y).  Whole tensors may exceed 2 GB (the
image base is a 64-bit pointer).  With a partial last channel tile the epilogue forms ((nb Cout + kb + r) H W + ...) * 4 for kb + r up
to Cout + 63 before it masks the lane, and the staging the same for the channels of a tail chunk: the channel counts carry a margin of
32 per image.  So: (C + 32) H W < 2^28, (K + 32) H W < 2^28 (hence H W < 2^23), 9 K C < 2^29, N H W < 2^31, CLHIP_EINVAL beyond.

The 64 MB cap of make_plan IS reachable without CLHIP_WG_SMALLC_BLOCKS.  splits = ceil(256 / tiles) is 2 for 128 <= tiles <= 255,
and a slab of 129..255 whole 64 x 64 tiles holds up to 9 * 4096 * 255 floats = 37.6 MB: two of them pass 64 MB as soon as
9 K C + K > 2^23 floats (K C > 932 067), e.g. (16, 960, 1024, 8, 8): 240 tiles, 16 stages / 2 >= 8 so not pixel-split, splits 2 -> 1
(CAP_CASE below; with tiles >= 256 the cap also `binds` but splits is 1 already).  Below 128 tiles the product slab * splits stays
below 9 * 4096 * tiles * (256 / tiles + 1) * 4 < 56 MB, and the first-layer kernel's below 28 K * 4 * (1024 / ceil(K / 64) + 1).  The
cap case needs 71 MB of workspace and 9 G multiply-adds of reference: it is pinned in the table and in the workspace sweep of the CPU
test, not on the GPU.

The `groups` slabs of ws_floats are never touched: bwd_weight_impl launches one wgrad_reduce_kernel over `splits` slabs, whose two
levels (16 contiguous ranges of slabs, then the 16 range sums) live in registers and LDS.  The GPU test pins that: exactly
splits * slab floats of the workspace change."""
from collections import namedtuple

KT = 64
BIG_MIN = 300
EINVAL, ENOSPC, ENOTSUP = -1, -2, -3

FwdPlan = namedtuple("FwdPlan", "kernel geo vec ck blocks n_a blocks_a")      # geo: (TW, TH, NB) or, mixed, (TW, THa, NBa, THb, NBb)
PoolPlan = namedtuple("PoolPlan", "kernel full gx kts ntiles")              # kernel c3w64 / c3; chunked rows carry a FwdPlan
WPlan = namedtuple("WPlan", "TW TH tiles_w tiles_h total_stages splits k_tiles c_tiles group groups ps slab ws_floats")
WgKernel = namedtuple("WgKernel", "name TW vec ps unpool")                  # name: c3_unpool / smallc / wgrad


def cdiv(a, b):
    return (a + b - 1) // b


def dims_ok(N, C, K, H, W):
    if min(N, C, K, H, W) <= 0:
        return False
    hw = H * W
    return hw < 1 << 23 and hw * (C + 32) < 1 << 28 and hw * (K + 32) < 1 << 28 and K * C < (1 << 29) // 9 and hw * N <= 0x7fffffff


# ------------------------------------------------------------------------------------------------ forward / backward-data
def vec_ok(Cin, H, W, Cw, aligned=True):
    """16-byte staging: `in` has Cin channels, the weight tensor's inner channel count is Cw (the layer's C), in | wt 16-byte aligned."""
    TW = 32 if W > 16 else (16 if W > 8 else 8)
    return Cin % 8 == 0 and Cw % 4 == 0 and W % 4 == 0 and W % TW == 0 and bool(aligned)


def fwd_vec(C, H, W, aligned=True):
    return C > 4 and vec_ok(C, H, W, C, aligned)


def bwd_vec(C, K, H, W, aligned=True):
    return vec_ok(K, H, W, C, aligned)


def launch_conv(N, Cin, Cout, H, W, vec, ck=8, pool=False, unpool=False):
    """launch_conv<CK, MODE, VEC, UNPOOL> on the KERNEL's channels."""
    kts = cdiv(Cout, KT)
    big = (N * H * W // 128) * kts >= BIG_MIN

    def geo(tw, th, nb):
        return FwdPlan("plain", (tw, th, nb), vec, ck, cdiv(W, tw) * cdiv(H, th) * cdiv(N, nb) * kts, N, None)
    if not vec and not unpool and H == 13 and W == 13 and not pool:
        return geo(13, 13, 1)._replace(kernel="dense")
    if vec and W > 16 and big:
        tw_n, tha, thb = cdiv(W, 32), cdiv(H, 4), cdiv(H, 2)
        per_img = tw_n * tha * kts
        total = per_img * N
        rem = total % 256
        if total > 256 and rem != 0 and rem <= 192:
            imgs_b = cdiv(rem, per_img)
            n_a = N - imgs_b
            if n_a > 0:
                blocks_a = per_img * n_a
                return FwdPlan("mixed", (32, 4, 1, 2, 1), vec, ck, blocks_a + tw_n * thb * kts * imgs_b, n_a, blocks_a)
    if vec and W <= 16 and big and H > 4:
        w16 = W > 8
        twx, nba = (16, 1) if w16 else (8, 2)
        tw_n, tha = cdiv(W, twx), cdiv(H, 8)
        thb = cdiv(H, 4) if w16 else cdiv(H, 8)
        per_unit = tw_n * tha * kts
        units = cdiv(N, nba)
        total = per_unit * units
        rem = total % 256
        if total >= 512 and rem != 0 and rem <= 192 and N % nba == 0:
            units_b = cdiv(rem, per_unit)
            n_a = (units - units_b) * nba
            if n_a > 0:
                blocks_a = per_unit * (units - units_b)
                g = (16, 8, 1, 4, 1) if w16 else (8, 8, 2, 8, 1)
                return FwdPlan("mixed2", g, vec, ck, blocks_a + tw_n * thb * kts * (N - n_a), n_a, blocks_a)
    if W > 16:
        return geo(32, 4, 1) if big else geo(32, 2, 1)
    if W > 8:
        return geo(16, 8, 1) if big else geo(16, 4, 1)
    return geo(8, 8, 2) if big and H > 4 else geo(8, 8, 1)


def fwd_plan(N, C, K, H, W, aligned=True, pool=False):
    """clhip_conv3x3_fwd, and the chunked arm of clhip_conv3x3_relu_pool_fwd (pool)."""
    if C <= 4:
        return launch_conv(N, C, K, H, W, False, 4, pool)
    return launch_conv(N, C, K, H, W, vec_ok(C, H, W, C, aligned), 8, pool)


def bwd_plan(N, C, K, H, W, aligned=True, unpool=False):
    """clhip_conv3x3_bwd_data / _bwd_data_unpool of the LAYER (N, C, K, H, W); ENOTSUP where the un-pooling entry refuses."""
    vec = vec_ok(K, H, W, C, aligned)
    if unpool and ((H | W) & 1 or not vec):
        return ENOTSUP
    return launch_conv(N, K, C, H, W, vec, 8, False, unpool)


# ------------------------------------------------------------------------------------------------ fused pooling, first layer
def c3w64_shape(N, C, K, H, W):
    return C == 3 and W % 64 == 0 and H % 2 == 0 and N * 3 * H * W < 1 << 29 and N * K * (H // 2) * (W // 2) < 1 << 29


def c3w64_gx(ntiles):
    return 256 if 256 * 8 <= 2 * ntiles else (2 * ntiles + 7) // 8


def pool_plan(N, C, K, H, W, aligned=True, out_aligned=True):
    """clhip_conv3x3_relu_pool_fwd on an even map.  out_aligned: y_pool and the codes both on a 16-byte boundary (the c3 kernel stores
    16 bytes at a time; the c3w64 and chunked kernels store dwords and bytes)."""
    assert not (H | W) & 1
    kts = cdiv(K, KT)
    if c3w64_shape(N, C, K, H, W):
        ntiles = (W // 64) * (H // 2) * N
        return PoolPlan("c3w64", K % KT == 0, c3w64_gx(ntiles), kts, ntiles)
    if C == 3 and W % 32 == 0 and out_aligned:
        ntiles = (W // 32) * cdiv(H, 8) * N
        return PoolPlan("c3", None, min(max(512 // kts, 1), ntiles), kts, ntiles)
    return fwd_plan(N, C, K, H, W, aligned, pool=True)


# ------------------------------------------------------------------------------------------------ weight gradient
def make_plan(N, C, K, H, W):
    TW, TH = (32, 2) if W > 16 else ((16, 4) if W > 8 else (8, 8))
    tiles_w, tiles_h = cdiv(W, TW), cdiv(H, TH)
    total = tiles_w * tiles_h * N
    smallc = C * 9 <= 32
    k_tiles, c_tiles, ps = cdiv(K, 64), (1 if smallc else cdiv(C, 64)), 0
    if not smallc:
        splits64 = cdiv(256, k_tiles * c_tiles)
        if total // splits64 < 8:
            ps, k_tiles, c_tiles = 1, cdiv(K, 32), cdiv(C, 32)
    splits = min(cdiv(1024 if smallc else 256, k_tiles * c_tiles), total)
    slab = 9 * K * C + K
    splits = max(min(splits, max((64 << 20) // (slab * 4), 1)), 1)
    group = 1
    while group * group < splits:
        group += 1
    groups = cdiv(splits, group)
    return WPlan(TW, TH, tiles_w, tiles_h, total, splits, k_tiles, c_tiles, group, groups, ps, slab, slab * (splits + groups))


def ws_bytes(N, C, K, H, W):
    return make_plan(N, C, K, H, W).ws_floats * 4 if dims_ok(N, C, K, H, W) else 0


def wg_kernel(N, C, K, H, W, pooled=False, x_al=True, dy_al=True, idx_al=16):
    """bwd_weight_impl behind its workspace check.  idx_al: the largest power of two (up to 16) the codes' address is a multiple of."""
    if pooled and (H | W) & 1:
        return ENOTSUP
    p = make_plan(N, C, K, H, W)
    if C * 9 <= 32:
        if pooled and p.TW == 32 and W % 32 == 0 and dy_al and idx_al >= 16 and N * K * H * W < 1 << 31 and N * C * H * W < 1 << 29:
            return WgKernel("c3_unpool", 32, None, None, True)
        return WgKernel("smallc", p.TW, None, None, pooled)
    vec = W % 4 == 0 and W % p.TW == 0 and x_al and dy_al
    if pooled and (not vec or idx_al < 2):
        return ENOTSUP
    return WgKernel("wgrad", p.TW, vec, bool(p.ps), pooled)


# ------------------------------------------------------------------------------------------------ case tables
P = FwdPlan
# Forward / backward-data: (N, Cin, Cout, H, W) as the KERNEL sees the channels and the hand-worked plan of the forward call (backward-
# data of the layer with the roles swapped takes the same geometry, with CK = 8).  kts = ceil(Cout / 64); big = (N H W // 128) * kts >= 300.
FWD_CASES = [
    # ---- mixed launches (VEC, big)
    # kts 1, 300 * 128 px: big; per_img = 1 * ceil(4/4) * 1 = 1, total 300, rem 44 -> 44 images as 32x2 tiles: n_a 256, 256 + 1*2*1*44 blocks
    ((300, 8, 64, 4, 32), P("mixed", (32, 4, 1, 2, 1), True, 8, 256 + 88, 256, 256)),
    # its neighbours with rem 0: N = 256 is NOT big ((256 * 128 // 128) * 1 = 256 < 300) and takes (32,2,1): 1 * 2 * 256 blocks;
    # N = 512 is big with total 512, rem 0: the plain (32,4,1) launch
    ((256, 8, 64, 4, 32), P("plain", (32, 2, 1), True, 8, 512, 256, None)),
    ((512, 8, 64, 4, 32), P("plain", (32, 4, 1), True, 8, 512, 512, None)),
    # kts 4, 130 * 128 px -> 130 * 4 = 520: big; per_unit = 1 * 1 * 4, 130 units, total 520, rem 8 -> 2 units as 16x4 tiles: n_a 128,
    # 512 + 1 * 2 * 4 * 2 blocks
    ((130, 8, 256, 8, 16), P("mixed2", (16, 8, 1, 4, 1), True, 8, 512 + 16, 128, 512)),
    # 260 * 64 px // 128 = 130, * 4 = 520: big; units of 2 images: 130, per_unit 4, total 520, rem 8 -> 2 units = 4 images one per tile:
    # n_a 256, 512 + 1 * 1 * 4 * 4 blocks
    ((260, 8, 256, 8, 8), P("mixed2", (8, 8, 2, 8, 1), True, 8, 512 + 16, 256, 512)),
    # an odd N of the same size: 261 * 64 // 128 = 130 -> big, 131 units, rem 12, but N % 2 != 0: plain (8,8,2), 131 * 4 blocks
    ((261, 8, 256, 8, 8), P("plain", (8, 8, 2), True, 8, 524, 261, None)),
    # ---- plain geometries, VEC.  Cout = 72: a second k-tile of 8 channels; Cin = 16: two whole chunks
    ((2, 16, 72, 4, 32), P("plain", (32, 2, 1), True, 8, 1 * 2 * 2 * 2, 2, None)),
    # 225 * 128 // 128 * 2 = 450: big; per_img 2, total 450, rem 194 > 192: no mixed launch
    ((225, 8, 72, 4, 32), P("plain", (32, 4, 1), True, 8, 450, 225, None)),
    ((2, 16, 72, 8, 16), P("plain", (16, 4, 1), True, 8, 1 * 2 * 2 * 2, 2, None)),
    # 150 * 128 // 128 * 2 = 300: big; total 300 < 512: no mixed launch
    ((150, 8, 72, 8, 16), P("plain", (16, 8, 1), True, 8, 300, 150, None)),
    ((3, 16, 72, 8, 8), P("plain", (8, 8, 1), True, 8, 3 * 2, 3, None)),
    # 301 * 64 // 128 = 150, * 2 = 300: big; 151 image pairs (the last holds one image), total 302 < 512
    ((301, 8, 72, 8, 8), P("plain", (8, 8, 2), True, 8, 302, 301, None)),
    # ---- plain geometries, scalar staging, ragged tiles in both directions, Cin % 8 != 0 (tail chunk), Cout = 70
    ((2, 12, 40, 7, 18), P("plain", (32, 2, 1), False, 8, 1 * 4 * 2 * 1, 2, None)),
    ((2, 10, 24, 6, 35), P("plain", (32, 2, 1), False, 8, 2 * 3 * 2 * 1, 2, None)),
    # 153 * 126 = 19278 px // 128 = 150, * 2 = 300: big
    ((153, 12, 70, 7, 18), P("plain", (32, 4, 1), False, 8, 1 * 2 * 153 * 2, 153, None)),
    ((3, 5, 70, 5, 9), P("plain", (16, 4, 1), False, 8, 1 * 2 * 3 * 2, 3, None)),
    # 427 * 45 = 19215 px // 128 = 150, * 2 = 300: big
    ((427, 5, 70, 5, 9), P("plain", (16, 8, 1), False, 8, 1 * 1 * 427 * 2, 427, None)),
    ((3, 10, 70, 9, 7), P("plain", (8, 8, 1), False, 8, 1 * 2 * 3 * 2, 3, None)),
    # 305 * 63 = 19215 px // 128 = 150, * 2 = 300: big; 153 image pairs x 2 row tiles x 2 k-tiles
    ((305, 10, 70, 9, 7), P("plain", (8, 8, 2), False, 8, 1 * 2 * 153 * 2, 305, None)),
    # big but H <= 4: stays on (8,8,1).  1200 * 32 // 128 = 300
    ((1200, 8, 64, 4, 8), P("plain", (8, 8, 1), True, 8, 1200, 1200, None)),
    # ---- Cin <= 4: forward stages CK = 4 (backward-data of the swapped layer: K = 3, CK = 8, scalar)
    ((2, 3, 40, 6, 16), P("plain", (16, 4, 1), False, 4, 1 * 2 * 2 * 1, 2, None)),
    ((2, 4, 70, 5, 33), P("plain", (32, 2, 1), False, 4, 2 * 3 * 2 * 2, 2, None)),
    # ---- the whole-plane 13 x 13 tile (scalar staging only: 13 % 4 != 0)
    ((2, 8, 24, 13, 13), P("dense", (13, 13, 1), False, 8, 2, 2, None)),
]
FWD_ARMS = ({("plain", g, v) for g in ((32, 2, 1), (32, 4, 1), (16, 4, 1), (16, 8, 1), (8, 8, 1), (8, 8, 2)) for v in (False, True)} |
            {("dense", (13, 13, 1), False), ("mixed", (32, 4, 1, 2, 1), True), ("mixed2", (16, 8, 1, 4, 1), True), ("mixed2", (8, 8, 2, 8, 1), True)})

# Fused pooling: (N, C, K, H, W) of the layer and the plan.  c3w64: ntiles = (W / 64) * (H / 2) * N row pairs of 64 columns, 2 units (channel
# halves) each, dealt to gx * 4 SIMDs x 2 waves; gx = 256 or ceil(2 ntiles / 8).  c3: ntiles = (W / 32) * ceil(H / 8) * N, gx = min(512 / kts, ntiles).
Q = PoolPlan
POOL_CASES = [
    ((1, 3, 64, 2, 64), Q("c3w64", True, 1, 1, 1)),                 # one tile: both image edges are padding; 2 units on 8 waves
    ((1, 3, 40, 2, 128), Q("c3w64", False, 1, 1, 2)),               # a halo between the two tiles of a row; K = 40: a partial tile
    ((3, 3, 70, 2, 64), Q("c3w64", False, 1, 2, 3)),                # 3 tiles: 6 units on 4 SIMDs (per 1, rem 2); K = 70: partial second tile
    ((5, 3, 64, 2, 64), Q("c3w64", True, 2, 1, 5)),                 # 5 tiles: gx = ceil(10 / 8) = 2, 10 units on 8 SIMDs
    ((2, 3, 64, 6, 128), Q("c3w64", True, 3, 1, 12)),               # 3 row pairs x 2 tiles x 2 images: halo rows and columns inside the image
    ((33, 3, 64, 64, 64), Q("c3w64", True, 256, 1, 1056)),          # 2112 units on 1024 SIMDs: per 2, rem 64 — the persistent loop
    ((2, 3, 64, 2, 32), Q("c3", None, 2, 1, 2)),                    # H = 2: one ragged 8-row tile per image
    ((2, 3, 40, 6, 32), Q("c3", None, 2, 1, 2)),
    ((2, 3, 70, 10, 32), Q("c3", None, 4, 2, 4)),                   # two row tiles, the second with 2 of 8 rows
    ((1, 3, 64, 2, 96), Q("c3", None, 3, 1, 3)),
    ((2, 3, 64, 6, 96), Q("c3", None, 6, 1, 6)),
    ((43, 3, 70, 10, 96), Q("c3", None, 256, 2, 258)),              # kts 2 -> gx 256 < 3 * 2 * 43 = 258 tiles: two blocks take a second tile
    # the chunked kernel with codes: C = 3 off the 32-column grid, C = 4
    ((2, 3, 40, 4, 16), P("plain", (16, 4, 1), False, 4, 2, 2, None)),
    ((2, 4, 70, 4, 32), P("plain", (32, 2, 1), False, 4, 1 * 2 * 2 * 2, 2, None)),
]
POOL_ARMS = {("c3w64", True), ("c3w64", False), ("c3", None), ("plain", (16, 4, 1)), ("plain", (32, 2, 1))}

# Weight gradient: (N, C, K, H, W), pooled, (x aligned, dy aligned, alignment of the codes), the kernel and (splits, workspace bytes).
# stages = ceil(W / TW) * ceil(H / TH) * N with (TW, TH) = (32,2) W > 16, (16,4) W > 8, (8,8); first layer (9 C <= 32): splits =
# min(ceil(1024 / ceil(K/64)), stages); others: t64 = ceil(K/64) ceil(C/64), splits64 = ceil(256 / t64), pixel-split (32 x 32 tiles) if
# stages // splits64 < 8, splits = min(ceil(256 / tiles), stages); ws = (9 K C + K) * (splits + ceil(splits / ceil(sqrt(splits)))) * 4.
K_ = WgKernel
AL = (True, True, 16)
WG_CASES = [
    # ---- first layer
    ((5, 3, 40, 6, 35), False, AL, K_("smallc", 32, None, None, False), (30, 1120 * 35 * 4)),      # 2 x 3 x 5 = 30 stages; slab 27*40+40; groups of 6: 5
    ((5, 3, 70, 7, 12), False, AL, K_("smallc", 16, None, None, False), (10, 1960 * 13 * 4)),      # 1 x 2 x 5 = 10 stages; groups of 4: 3
    ((5, 2, 40, 9, 7), False, AL, K_("smallc", 8, None, None, False), (10, 760 * 13 * 4)),         # C = 2: slab 18 * 40 + 40
    # K odd, C even: slab 18 * 37 + 37 = 703, no multiple of 4 -> slabs off a 16-byte boundary, the reduction's scalar loads and its
    # ragged last thread (703 = 10 * 64 + 63)
    ((5, 2, 37, 9, 7), False, AL, K_("smallc", 8, None, None, False), (10, 703 * 13 * 4)),
    ((94, 3, 16, 32, 32), False, AL, K_("smallc", 32, None, None, False), (1024, 448 * (1024 + 32) * 4)),   # 1504 stages: 480 blocks take 2, the rest 1
    ((4, 3, 64, 8, 32), True, AL, K_("c3_unpool", 32, None, None, True), (16, 1792 * 20 * 4)),     # 1 x 4 x 4 = 16 stages
    ((4, 3, 40, 8, 64), True, AL, K_("c3_unpool", 32, None, None, True), (32, 1120 * 38 * 4)),     # two tiles per row, K = 40
    ((4, 3, 64, 8, 32), True, (True, False, 16), K_("smallc", 32, None, None, True), (16, 1792 * 20 * 4)),   # dy off 16 bytes
    ((4, 3, 64, 8, 32), True, (True, True, 2), K_("smallc", 32, None, None, True), (16, 1792 * 20 * 4)),     # codes off 16 bytes
    ((4, 3, 64, 8, 32), True, (True, True, 1), K_("smallc", 32, None, None, True), (16, 1792 * 20 * 4)),     # codes at an odd address
    ((4, 3, 64, 6, 40), True, AL, K_("smallc", 32, None, None, True), (24, 1792 * 29 * 4)),        # W % 32 != 0: 2 x 3 x 4 = 24 stages
    ((4, 3, 64, 8, 16), True, AL, K_("smallc", 16, None, None, True), (8, 1792 * 11 * 4)),         # TW = 16
    ((4, 2, 40, 8, 8), True, AL, K_("smallc", 8, None, None, True), (4, 760 * 6 * 4)),             # TW = 8
    # ---- pixel-split kernel.  K = 40, C = 24: t64 = 1, splits64 = 256; 32 x 32 tiles: 2 x 1 -> splits = min(128, stages); slab 8680
    ((200, 24, 40, 8, 8), False, AL, K_("wgrad", 8, True, True, False), (128, 8680 * 139 * 4)),    # 200 stages: 72 blocks take 2, 56 take 1
    ((300, 24, 40, 8, 8), False, AL, K_("wgrad", 8, True, True, False), (128, 8680 * 139 * 4)),    # 300 stages: 44 blocks take 3, 84 take 2
    ((300, 24, 40, 8, 8), True, AL, K_("wgrad", 8, True, True, True), (128, 8680 * 139 * 4)),
    ((9, 24, 40, 9, 7), False, AL, K_("wgrad", 8, False, True, False), (18, 8680 * 22 * 4)),       # 1 x 2 x 9 = 18 stages of one each
    ((20, 24, 40, 8, 16), False, AL, K_("wgrad", 16, True, True, False), (40, 8680 * 46 * 4)),
    ((20, 24, 40, 8, 16), True, AL, K_("wgrad", 16, True, True, True), (40, 8680 * 46 * 4)),
    ((5, 24, 40, 7, 12), False, AL, K_("wgrad", 16, False, True, False), (10, 8680 * 13 * 4)),
    # K = 37: slab 9 * 37 * 24 + 37 = 8029 = 4 * 2007 + 1 (the reduction's scalar loads; 8029 = 125 * 64 + 29: a ragged last block); 10 stages
    ((5, 24, 37, 7, 12), False, AL, K_("wgrad", 16, False, True, False), (10, 8029 * 13 * 4)),
    ((10, 24, 40, 4, 32), False, AL, K_("wgrad", 32, True, True, False), (20, 8680 * 24 * 4)),
    ((10, 24, 40, 4, 32), True, AL, K_("wgrad", 32, True, True, True), (20, 8680 * 24 * 4)),
    ((3, 24, 40, 5, 35), False, AL, K_("wgrad", 32, False, True, False), (18, 8680 * 22 * 4)),      # 2 x 3 x 3 = 18
    ((20, 24, 40, 8, 16), False, (False, True, 16), K_("wgrad", 16, False, True, False), (40, 8680 * 46 * 4)),     # x off: scalar staging
    # whole 32-channel tiles on every wave: K = C = 64 -> 2 x 2 tiles, splits 64; 100 stages: 36 blocks take 2
    ((100, 64, 64, 8, 8), False, AL, K_("wgrad", 8, True, True, False), (64, 36928 * 72 * 4)),
    # ---- 64 x 64-tile kernel: stages // splits64 >= 8.  K = 24, C = 12: one tile, splits 256, 2050 stages: 8 per block, two blocks 9; slab 2616
    ((2050, 12, 24, 8, 8), False, AL, K_("wgrad", 8, True, False, False), (256, 2616 * 272 * 4)),
    ((2050, 12, 24, 8, 8), True, AL, K_("wgrad", 8, True, False, True), (256, 2616 * 272 * 4)),
    ((2050, 12, 24, 8, 6), False, AL, K_("wgrad", 8, False, False, False), (256, 2616 * 272 * 4)),
    ((1025, 12, 24, 8, 16), False, AL, K_("wgrad", 16, True, False, False), (256, 2616 * 272 * 4)),
    ((1025, 12, 24, 8, 16), True, AL, K_("wgrad", 16, True, False, True), (256, 2616 * 272 * 4)),
    ((1025, 12, 24, 8, 12), False, AL, K_("wgrad", 16, False, False, False), (256, 2616 * 272 * 4)),
    ((1025, 12, 24, 4, 32), False, AL, K_("wgrad", 32, True, False, False), (256, 2616 * 272 * 4)),
    ((1025, 12, 24, 4, 32), True, AL, K_("wgrad", 32, True, False, True), (256, 2616 * 272 * 4)),
    ((1025, 12, 24, 4, 20), False, AL, K_("wgrad", 32, False, False, False), (256, 2616 * 272 * 4)),
    # all four waves of the 64 x 64 tile at work: K = C = 72 -> 2 x 2 tiles, splits64 = 64, 512 stages // 64 = 8; slab 46728
    ((512, 72, 72, 8, 8), False, AL, K_("wgrad", 8, True, False, False), (64, 46728 * 72 * 4)),
]
WG_ARMS = ({K_("smallc", tw, None, None, u) for tw in (32, 16, 8) for u in (False, True)} | {K_("c3_unpool", 32, None, None, True)} |
           {K_("wgrad", tw, v, ps, False) for tw in (32, 16, 8) for v in (False, True) for ps in (False, True)} |
           {K_("wgrad", tw, True, ps, True) for tw in (32, 16, 8) for ps in (False, True)})
# The pixel-split switch at full tiles (table only: 47 MB of workspace and 4.8 G multiply-adds of reference each): t64 = 16, splits64 = 16,
# 4 stages per image: 124 // 16 = 7 -> pixel-split on 8 x 8 tiles of 32 x 32, splits 4; 128 // 16 = 8 -> 64 x 64 tiles, splits 16
PS_SWITCH = [((31, 256, 256, 16, 16), 1, 4), ((32, 256, 256, 16, 16), 0, 16)]
# 3 x 3 tiles of 64 x 64 (tile indices beyond 2 x 2, partial third tiles of 8 channels): t64 = 9, splits64 = ceil(256 / 9) = 29,
# 234 stages // 29 = 8: not pixel-split, splits 29 (2 blocks take 9 stages, 27 take 8); slab 9 * 136 * 136 + 136 = 166600, groups of 6: 5.
# 22.7 MB of workspace: the GPU test runs it on exactly that (test_weight_gradient_three_by_three_tiles), not on twice as WG_CASES' rows.
TILES_3X3 = ((234, 136, 136, 8, 8), False, AL, K_("wgrad", 8, True, False, False), (29, 166600 * 34 * 4))
# The 64 MB cap (see the header): 16 x 15 = 240 tiles -> splits 2, slab 35.4 MB -> 1
CAP_CASE = ((16, 960, 1024, 8, 8), 1, (9 * 1024 * 960 + 1024) * 2 * 4)
# ENOTSUP of the un-pooling weight gradient: (shape, alignment) -> refused
WG_REFUSED = [((4, 24, 40, 7, 8), AL), ((4, 24, 40, 8, 7), AL), ((4, 3, 40, 7, 32), AL),          # odd maps, general and first layer
              ((4, 24, 40, 8, 12), AL), ((4, 24, 40, 8, 6), AL),                                     # no 16-byte staging: W % TW, W % 4
              ((4, 24, 40, 8, 8), (False, True, 16)), ((4, 24, 40, 8, 8), (True, False, 16)),         # x or dy off a 16-byte boundary
              ((4, 24, 40, 8, 8), (True, True, 1))]                                                  # codes at an odd address


def check_case_tables():
    arms, cks = set(), set()
    for shape, plan in FWD_CASES:
        assert dims_ok(shape[0], shape[1], shape[2], *shape[3:])
        got = fwd_plan(*shape)
        assert got == plan, (shape, got, plan)
        arms.add((plan.kernel, plan.geo, plan.vec))
        cks.add(plan.ck)
        N, Cin, Cout, H, W = shape                         # backward-data of the swapped layer: the same geometry, CK = 8
        b = bwd_plan(N, Cout, Cin, H, W)
        if Cin % 8 == 0 or not plan.vec:
            assert b == plan._replace(ck=8, vec=bwd_vec(Cout, Cin, H, W)) and (b.vec == plan.vec or Cin <= 4), (shape, b)
    assert arms == FWD_ARMS, (FWD_ARMS - arms, arms - FWD_ARMS)
    assert cks == {4, 8}
    assert any(s[1] % 8 and s[1] > 8 for s, _ in FWD_CASES) and any(s[2] % 64 and s[2] > 64 for s, _ in FWD_CASES)
    arms = set()
    for shape, plan in POOL_CASES:
        got = pool_plan(*shape)
        assert got == plan, (shape, got, plan)
        arms.add((plan.kernel, plan.full) if isinstance(plan, PoolPlan) else (plan.kernel, plan.geo))
    assert arms == POOL_ARMS, (POOL_ARMS - arms, arms - POOL_ARMS)
    assert any(isinstance(p, PoolPlan) and p.kernel == "c3" and p.ntiles > p.gx for _, p in POOL_CASES)
    arms, per_block = set(), set()
    assert {k.name for s, _, _, k, _ in WG_CASES if make_plan(*s).slab % 4} == {"smallc", "wgrad"}     # slabs off a 16-byte boundary: the reduction's scalar arm
    p = make_plan(*TILES_3X3[0])
    assert (p.ps, p.k_tiles, p.c_tiles, p.total_stages % p.splits) == (0, 3, 3, 2)
    for shape, pooled, al, kern, (splits, nbytes) in WG_CASES + [TILES_3X3]:
        p = make_plan(*shape)
        assert wg_kernel(*shape, pooled, *al) == kern, (shape, pooled, al, wg_kernel(*shape, pooled, *al))
        assert (p.splits, ws_bytes(*shape)) == (splits, nbytes), (shape, p.splits, ws_bytes(*shape))
        arms.add(kern)
        if kern.name == "wgrad" and p.total_stages % p.splits:
            per_block.add(p.total_stages // p.splits)
    assert arms == WG_ARMS, (WG_ARMS - arms, arms - WG_ARMS)
    assert {1, 2} <= per_block                              # blocks of 1 and 2, of 2 and 3 stages in one launch (the pipeline's prologue / epilogue)
    for shape, ps, splits in PS_SWITCH:
        p = make_plan(*shape)
        assert (p.ps, p.splits) == (ps, splits), (shape, p)
    shape, splits, nbytes = CAP_CASE
    p = make_plan(*shape)
    assert not p.ps and p.k_tiles * p.c_tiles == 240 and 2 * p.slab * 4 > 64 << 20 and (p.splits, ws_bytes(*shape)) == (splits, nbytes)
    for shape, al in WG_REFUSED:
        assert wg_kernel(*shape, True, *al) == ENOTSUP, (shape, al)
