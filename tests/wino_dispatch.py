"""The launch decisions of csrc/wino.hip restated in Python (test infrastructure shared by test_wino_args_cpu.py and
test_gpu_wino_kernels.py).  Nothing here calls the library; the tests compare what the library does with these rules.

Forward and backward-data run the SAME kernels: the kernel's (Cin, Cout) is the layer's (C, K) forward and (K, C) backward-data.
launch_wino picks, at the default CLHIP_WINO16_BELOW_UNITS = 640:
  conv16  <KT2>          wino_conv16_kernel      8 x 8 maps with fewer than 640 units of ceil(16 N / 32) * ceil(Cout / 32);
                                                 KT2 = 1 (one image x 64 channels per block) while N * ceil(Cout / 32) <= 512, else 2
  conv16g <TC, TR, ER>   wino_conv16g_kernel     <8,2,1> odd maps 9..16 wide (row-packed), <8,2,4> even maps >= 16 wide,
                                                 <4,4,4> the other 8 x 8 maps
  conv32                 wino_conv_kernel        what is left: even maps narrower than 16 other than 8 x 8
The weight gradient (wino_wgrad_geo): `wide` (W >= 16) picks the 8 x 2-tile stage over the 4 x 4 one, `vec` (W a whole number of
stages wide and x | dy 16-byte aligned) the 16-byte staging, `ps` (fewer than 16 stages per block of the 64 x 64-tile kernel) the
pixel-split kernel on 32 x 32 tiles; the split count is capped by the workspace the caller hands over."""
from collections import namedtuple

WKT, WCK, WFP = 64, 8, 20
W_FLOATS = WCK * WKT * WFP                  # LDS image of one 8-channel chunk of one 64-channel k-tile
WD_FLOATS = 4 * WKT * 16                    # lane-ordered image of one 4-channel chunk
WU_FLOATS = W_FLOATS + 2 * WD_FLOATS
BELOW_UNITS = 640
PAIR_MAX_PIXELS = 256
MAX_ELEMS = 1 << 29                         # N*K*H*W and N*C*H*W of the weight gradient stay BELOW this (32-bit byte offsets)
EINVAL, ENOSPC, ENOTSUP = -1, -2, -3

FwdPlan = namedtuple("FwdPlan", "kernel targs blocks")
WgradGeo = namedtuple("WgradGeo", "ps wide vec splits tiles")            # tiles: 32 x 32 (k, c) tiles if ps, else 64 x 64
PairPlan = namedtuple("PairPlan", "dk tc tr nb_d nb_w splits")


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ forward / backward-data
def wino_ok(Cin, Cout, H, W):
    if Cin % WCK or Cin < 16 or Cout % 32 or H < 4 or W < 8:
        return False
    if (H | W) & 1 == 0:
        return True
    return 8 < W <= 16


def wino_ws_bytes(Cin, Cout):
    return cdiv(Cout, WKT) * cdiv(Cin, WCK) * WU_FLOATS * 4


def conv3x3_wino_ws(C, K):
    return max(wino_ws_bytes(C, K), wino_ws_bytes(K, C))


def units(N, Cout):
    return cdiv(N * 16, 32) * cdiv(Cout, 32)


def fwd_plan(N, Cin, Cout, H, W):
    """launch_wino for a shape of wino_ok (None outside it)."""
    if N <= 0 or not wino_ok(Cin, Cout, H, W):
        return None
    kts = cdiv(Cout, WKT)
    if H == 8 and W == 8 and units(N, Cout) < BELOW_UNITS:
        narrow = N * cdiv(Cout, 32) <= 512
        return FwdPlan("conv16", (1 if narrow else 2,), (N if narrow else cdiv(N, 2)) * kts)

    def g16(tc, tr, er):
        tiles_w, groups, ne = cdiv(cdiv(W, 2), tc), cdiv(cdiv(H, 2), er), 2 * tr // er
        return FwdPlan("conv16g", (tc, tr, er), cdiv(N * groups, ne) * tiles_w * kts)
    if (H | W) & 1:
        assert W <= 16                              # wino_ok
        return g16(8, 2, 1)
    if W >= 16:
        return g16(8, 2, 4)
    if H == 8 and W == 8:
        return g16(4, 4, 4)
    return FwdPlan("conv32", (), cdiv(cdiv(W, 2), 4) * cdiv(cdiv(H, 2), 4) * cdiv(N, 4) * kts)


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad_ok(C, K, H, W):
    return C % WKT == 0 and K % WKT == 0 and C > 0 and K > 0 and H >= 4 and W >= 8


def slab_floats(C, K):
    return 9 * K * C + K


def wgrad_ws_bytes(N, C, K, H, W):
    """clhip_internal_wino_wgrad_ws: the slabs the launch wants (it takes fewer when the workspace is smaller)."""
    if N <= 0 or not wgrad_ok(C, K, H, W):
        return 0
    kc_tiles = (K // WKT) * (C // WKT)
    return slab_floats(C, K) * cdiv(256, kc_tiles) * 4


def wgrad_stages(N, H, W):
    wide = W >= 16
    tcs, trs = (8, 2) if wide else (4, 4)
    return cdiv(cdiv(W, 2), tcs) * cdiv(cdiv(H, 2), trs) * N


def wgrad_geo(N, C, K, H, W, ws_bytes, aligned=True, pooled=False):
    """wino_wgrad_geo: a WgradGeo, or ENOTSUP / ENOSPC.  aligned: x and dy both on a 16-byte boundary."""
    if not wgrad_ok(C, K, H, W):
        return ENOTSUP
    if N * K * H * W >= MAX_ELEMS or N * C * H * W >= MAX_ELEMS:
        return ENOTSUP
    wide = W >= 16
    tcs = 8 if wide else 4
    if (H | W) & 1 and pooled:
        return ENOTSUP
    total = wgrad_stages(N, H, W)
    if total > 0x7fffffff:
        return ENOTSUP
    kc_tiles = (K // WKT) * (C // WKT)
    splits = 1 if kc_tiles >= 256 else 256 // kc_tiles
    splits = min(splits, total)
    cap = ws_bytes // (slab_floats(C, K) * 4)
    if cap < 1:
        return ENOSPC
    splits = min(splits, cap)
    vec = W % (2 * tcs) == 0 and bool(aligned)
    kc32 = (K // 32) * (C // 32)
    ps = total < 16 * splits
    if not ps:
        return WgradGeo(False, wide, vec, splits, kc_tiles)
    target = 256 if H * W <= 64 and kc32 <= 16 else 512
    sp = 1 if kc32 >= target else target // kc32
    return WgradGeo(True, wide, vec, min(sp, total, cap), kc32)


# ------------------------------------------------------------------------------------------------ merged backward grid
def bwd_u_bytes(C, K):
    return (wino_ws_bytes(K, C) + 255) & ~255


def wino_bwd_ws_bytes(N, C, K, H, W):
    slabs = wgrad_ws_bytes(N, C, K, H, W)
    return bwd_u_bytes(C, K) + slabs if slabs else 0


def pair_plan(N, C, K, H, W, pooled=False, ws_bytes=1 << 40, aligned=True):
    """clhip_internal_wino_pair on `ws_bytes` of slab workspace: a PairPlan, or None where it answers CLHIP_ENOTSUP."""
    if N <= 0 or (H | W) & 1 or H * W > PAIR_MAX_PIXELS or not wino_ok(K, C, H, W):
        return None
    wide, m88 = W >= 16, H == 8 and W == 8
    if not wide and not m88:
        return None
    g = wgrad_geo(N, C, K, H, W, ws_bytes, aligned, pooled)
    if not isinstance(g, WgradGeo) or not g.ps or not g.vec or g.wide != wide:
        return None
    tc, tr = (8, 2) if wide else (4, 4)
    ne = 2 * tr // 4
    narrow = m88 and units(N, C) < BELOW_UNITS and N * cdiv(C, 32) <= 512
    npb = N if narrow else cdiv(N * cdiv(H // 2, 4), ne) * cdiv(W // 2, tc)
    return PairPlan(1 if narrow else 0, tc, tr, npb * cdiv(C, WKT), g.tiles * g.splits, g.splits)


def pair_shape(N, C, K, H, W, pooled=False):
    """clhip_internal_wino_pair_shape: the plan-time form (aligned tensors, enough workspace)."""
    return pair_plan(N, C, K, H, W, pooled) is not None


# ------------------------------------------------------------------------------------------------ case tables
# Forward / backward-data: (N, Cin, Cout, H, W) as the KERNEL sees the channels, and the hand-worked plan.
#   units(N, Cout) = ceil(16 N / 32) * ceil(Cout / 32);  conv16g blocks = ceil(N * groups / NE) * tiles_w * ceil(Cout / 64)
FWD_CASES = [
    # 8 x 8, 2 units, 3 * 1 <= 512: one image x 64 channels per block, Cout = 32 fills half of the one k-tile
    ((3, 16, 32, 8, 8), FwdPlan("conv16", (1,), 3)),
    # 17 * 16 = 272 units; 33 * 16 = 528 > 512: two images per block, 17 image pairs (the last holds one image) x 8 k-tiles
    ((33, 16, 512, 8, 8), FwdPlan("conv16", (2,), 136)),
    # ceil(16 * 78 / 32) = 39 -> 624 units: the last N below the switch at Cout = 512
    ((78, 16, 512, 8, 8), FwdPlan("conv16", (2,), 312)),
    # ceil(16 * 79 / 32) = 40 -> 640 units, NOT below: the smallest N on the 16-tile kernel (40 image pairs, the last with one image)
    ((79, 16, 512, 8, 8), FwdPlan("conv16g", (4, 4, 4), 320)),
    ((80, 16, 512, 8, 8), FwdPlan("conv16g", (4, 4, 4), 320)),             # 640 units exactly, whole image pairs
    # even maps >= 16 wide; Cin = 24 = three 8-channel chunks, Cout = 96 = 1.5 k-tiles (2 k-tiles of blocks)
    ((3, 24, 96, 4, 16), FwdPlan("conv16g", (8, 2, 4), 6)),                # minimum H: half of the entity's four tile rows
    ((3, 24, 96, 6, 18), FwdPlan("conv16g", (8, 2, 4), 12)),               # 3 of 4 tile rows, second column block is one tile wide
    ((3, 24, 96, 10, 32), FwdPlan("conv16g", (8, 2, 4), 24)),              # two row groups (4 + 1 tile rows) x two full column blocks
    # odd maps 9..16 wide, row-packed: entity = one tile row, four per block; N * ceil(H / 2) = 9, 6, 21 leave the last block ragged
    ((3, 16, 32, 5, 9), FwdPlan("conv16g", (8, 2, 1), 3)),
    ((3, 16, 32, 4, 15), FwdPlan("conv16g", (8, 2, 1), 2)),
    ((3, 16, 32, 13, 16), FwdPlan("conv16g", (8, 2, 1), 6)),
    ((3, 16, 32, 7, 10), FwdPlan("conv16g", (8, 2, 1), 3)),                # ceil(7 / 2) = 4: every N fills whole blocks here
    # even maps narrower than 16 other than 8 x 8: 4 x 4 tiles of 4 images per block, N = 5 leaves a group of one image
    ((5, 16, 32, 4, 8), FwdPlan("conv32", (), 2)),
    ((5, 16, 32, 6, 10), FwdPlan("conv32", (), 4)),
    ((5, 16, 32, 12, 12), FwdPlan("conv32", (), 8)),
    ((5, 16, 32, 8, 14), FwdPlan("conv32", (), 4)),
]
FWD_ARMS = {("conv16", (1,)), ("conv16", (2,)), ("conv16g", (8, 2, 4)), ("conv16g", (4, 4, 4)), ("conv16g", (8, 2, 1)), ("conv32", ())}

# (Cin, Cout, H, W) outside wino_ok, and why
REFUSED = [
    (16, 32, 5, 8), (16, 32, 7, 8),                        # W = 8 with odd H
    (16, 32, 13, 17), (16, 32, 8, 17), (16, 32, 21, 21),   # odd maps wider than 16
    (16, 32, 9, 7), (16, 32, 5, 7),                        # odd maps narrower than 9: W = 8 above, below it W < 8 refuses as well
    (8, 32, 8, 8), (20, 32, 8, 8), (16, 48, 8, 8), (16, 16, 8, 8), (0, 32, 8, 8),   # Cin = 8, Cin % 8, Cout % 32
    (16, 32, 2, 8), (16, 32, 3, 9), (16, 32, 8, 6),        # H = 2, H = 3, W = 6
]

# Weight gradient: (N, C, K, H, W), pooled, slabs of workspace handed over (None: what wgrad_ws_bytes asks for), aligned,
# and the hand-worked WgradGeo.  stages = ceil(ceil(W/2) / TCS) * ceil(ceil(H/2) / TRS) * N with (TCS, TRS) = (8, 2) wide, (4, 4) narrow.
WG_CASES = [
    # ---- pixel-split kernel: stages < 16 * splits.  64 -> 64: 1 tile of 64 x 64, 4 of 32 x 32; splits = min(target / 4, stages)
    ((2, 64, 64, 8, 8), False, None, True, WgradGeo(True, False, True, 2, 4)),         # 2 stages
    ((2, 64, 64, 8, 8), True, None, True, WgradGeo(True, False, True, 2, 4)),
    ((2, 64, 64, 4, 16), False, None, True, WgradGeo(True, True, True, 2, 4)),         # wide: 1 x 1 stage per image
    ((2, 64, 64, 4, 16), True, None, True, WgradGeo(True, True, True, 2, 4)),
    ((2, 64, 64, 12, 12), False, None, True, WgradGeo(True, False, False, 8, 4)),      # 12 % 8: scalar; 2 x 2 x 2 = 8 stages
    ((2, 64, 64, 12, 12), True, None, True, WgradGeo(True, False, False, 8, 4)),
    ((2, 64, 64, 6, 18), False, None, True, WgradGeo(True, True, False, 8, 4)),        # 18 % 16: scalar; 2 x 2 x 2 = 8 stages
    ((2, 64, 64, 6, 18), True, None, True, WgradGeo(True, True, False, 8, 4)),
    ((2, 64, 64, 5, 9), False, None, True, WgradGeo(True, False, False, 4, 4)),        # odd: 2 x 1 x 2 = 4 stages
    ((2, 64, 64, 13, 13), False, None, True, WgradGeo(True, False, False, 8, 4)),      # odd: 2 x 2 x 2 = 8 stages
    ((2, 128, 64, 8, 8), False, None, True, WgradGeo(True, False, True, 2, 8)),        # kc32 = 8
    ((2, 64, 128, 8, 8), False, None, True, WgradGeo(True, False, True, 2, 8)),
    ((2, 64, 64, 8, 8), False, None, False, WgradGeo(True, False, False, 2, 4)),       # x or dy off a 16-byte boundary: scalar
    ((2, 64, 64, 4, 16), False, None, False, WgradGeo(True, True, False, 2, 4)),
    ((3, 64, 64, 8, 8), False, 1, True, WgradGeo(True, False, True, 1, 4)),            # 3 stages < 16 on one slab: still pixel-split
    # ---- wino_wgrad_kernel: stages >= 16 * splits, reached by handing over one slab (or two)
    ((4, 64, 64, 16, 16), False, 1, True, WgradGeo(False, True, True, 1, 1)),          # 1 x 4 x 4 = 16 stages
    ((4, 64, 64, 16, 16), True, 1, True, WgradGeo(False, True, True, 1, 1)),
    ((16, 64, 64, 8, 8), False, 1, True, WgradGeo(False, False, True, 1, 1)),          # 16 stages
    ((16, 64, 64, 8, 8), True, 1, True, WgradGeo(False, False, True, 1, 1)),
    ((4, 64, 64, 12, 12), False, 1, True, WgradGeo(False, False, False, 1, 1)),        # 2 x 2 x 4 = 16 stages, scalar
    ((4, 64, 64, 12, 12), True, 1, True, WgradGeo(False, False, False, 1, 1)),
    ((4, 64, 64, 6, 18), False, 1, True, WgradGeo(False, True, False, 1, 1)),          # 2 x 2 x 4 = 16 stages, wide scalar
    ((4, 64, 64, 6, 18), True, 1, True, WgradGeo(False, True, False, 1, 1)),
    ((4, 64, 64, 13, 13), False, 1, True, WgradGeo(False, False, False, 1, 1)),        # odd map: 2 x 2 x 4 = 16 stages
    ((8, 64, 64, 16, 16), False, 2, True, WgradGeo(False, True, True, 2, 1)),          # 32 stages, room for two slabs
    ((4, 64, 64, 16, 16), False, 1, False, WgradGeo(False, True, False, 1, 1)),        # misaligned: the scalar form of the same kernel
    ((4, 64, 64, 16, 16), False, 2, True, WgradGeo(True, True, True, 2, 4)),           # 16 < 32: two slabs send it back to pixel-split
]
WG_ARMS = {(ps, wide, vec, pooled) for ps in (False, True) for wide in (False, True) for vec in (False, True) for pooled in (False, True)}

# Merged backward grid: (N, C, K, H, W) of the LAYER and the plan, the same plain and pooled.
PAIR_CASES = [
    # wide: backward-data 3 images x 2 row groups x 1 column block x 1 k-tile = 6 blocks; 12 stages -> 12 splits x 4 tiles
    ((3, 64, 64, 16, 16), PairPlan(0, 8, 2, 6, 48, 12)),
    # 8 x 8, 2 * 2 = 4 units, 3 * 2 <= 512: one-image blocks; 3 stages -> 3 splits x 4 tiles
    ((3, 64, 64, 8, 8), PairPlan(1, 4, 4, 3, 12, 3)),
    # 8 x 8, 272 units but 33 * 16 > 512: the grid runs the conv16g body on 17 image pairs x 8 k-tiles where launch_wino runs
    # conv16<2>; kc32 = 32 -> 512 / 32 = 16 splits
    ((33, 512, 64, 8, 8), PairPlan(0, 4, 4, 136, 512, 16)),
]
PAIR_DECLINED = [(200, 64, 64, 32, 32, True), (8, 64, 64, 12, 12, False), (8, 64, 64, 13, 13, False), (8, 64, 64, 32, 16, False),
                 (4, 48, 64, 16, 16, False)]         # what test_one_grid_backward_declines_other_shapes lists


def wg_ws_bytes(case):
    shape, pooled, slabs, aligned, geo = case
    N, C, K, H, W = shape
    return wgrad_ws_bytes(*shape) if slabs is None else slabs * slab_floats(C, K) * 4


def check_case_table():
    arms = set()
    for shape, plan in FWD_CASES:
        N, Cin, Cout, H, W = shape
        assert wino_ok(Cin, Cout, H, W), shape
        assert fwd_plan(*shape) == plan, (shape, fwd_plan(*shape), plan)
        arms.add((plan.kernel, plan.targs))
    assert arms == FWD_ARMS, FWD_ARMS - arms
    for s in REFUSED:
        assert not wino_ok(*s) and fwd_plan(1, *s) is None, s
    arms = set()
    for case in WG_CASES:
        shape, pooled, slabs, aligned, geo = case
        got = wgrad_geo(*shape, wg_ws_bytes(case), aligned, pooled)
        assert got == geo, (case, got)
        assert geo.ps or wgrad_stages(shape[0], *shape[3:]) >= 16 * geo.splits
        arms.add((geo.ps, geo.wide, geo.vec, pooled))
    assert arms == WG_ARMS, WG_ARMS - arms
    arms = set()
    for shape, plan in PAIR_CASES:
        for pooled in (False, True):
            assert pair_plan(*shape, pooled) == plan and pair_shape(*shape, pooled), (shape, pair_plan(*shape, pooled))
        arms.add((plan.dk, plan.tc, plan.tr))
    assert arms == {(0, 8, 2), (1, 4, 4), (0, 4, 4)}
    N, C, K, H, W = PAIR_CASES[2][0]                       # the documented exception: the two launches run conv16<2> there
    assert fwd_plan(N, K, C, H, W) == FwdPlan("conv16", (2,), 136)
    for s in PAIR_DECLINED:
        assert not pair_shape(*s), s
