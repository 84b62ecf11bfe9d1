"""The launch rules of the bf16-split 3x3 kernels, restated from csrc/bsconv.hip (clhip_conv3x3_bs_fwd / _bs_bwd_data), csrc/bswgrad.hip
(clhip_conv3x3_bs_bwd_weight on whole 16-pixel strips) and the 3x3 instance of csrc/bswgrad5.hip (the tap-split kernel that takes the
other maps) — test infrastructure, plain Python.  Every table row below was worked out by hand from the conditions in the sources;
check_tables() recomputes each from the functions here, test_bs_args_cpu.py holds the functions against the library, and
test_gpu_bs3x3_kernels.py runs the rows.

Shapes are (N, C, K, H, W) of the LAYER.  The kernels see (Cin, Cout) = (C, K) on the forward and (K, C) on backward-data.

Rows of the issue that the restated rules correct:
  * per-byte tail of the pooled code store.  The tail (pw + PW > OW) lies inside the fast epilogue, which needs OW % 4 == 0; W = 4, 12, 20
    have OW = 2, 6, 10 and take the general (window) epilogue instead.  A wave's pooled region is PW = 4 / 8 / 16 codes wide in the
    8- / 16- / 32-wide geometry and the 8- and 16-wide geometries only ever see OW == PW, so the tail is reachable only for W > 16 with
    OW % 16 in (4, 8, 12): rows (1, 32, 64, 4, 24) (the whole code row is the tail) and (1, 32, 64, 4, 40) (a b128 store and a tail in the
    same row) were added for it (and the mixed-grid family has W = 24: PW = 8 in its GB tiles).
  * (3,128,64,7,16) and (5,64,128,6,48) have rows = 21 and 90 below their 256 / tiles = 128 slabs: every share is ONE row (extra = 0).
    They stay (one-row shares across strips and images); (3,256,256,7,16) and (3,128,256,5,48) were added: splits 16 and 32 below
    rows 21 and 45, shares of two rows and of one that cross an image and a strip boundary."""

EINVAL, ENOSPC, ENOTSUP = -1, -2, -3
BS_BN, BS_CK = 64, 16
LIMIT = 0x7fffffff


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ forward / backward-data
def kernel_view(kind, C, K):
    """(Cin, Cout) as bs_conv_body sees them."""
    return (C, K) if kind == "fwd" else (K, C)


def bs_ok(Cin, Cout, H, W):
    """clhip_internal_bs_ok."""
    return Cin >= 32 and Cin % 32 == 0 and Cout >= 64 and Cout % 64 == 0 and H >= 4 and W >= 4


def image_bytes(Cin, Cout, ks=3):
    """clhip_internal_bs_ws / clhip_internal_bs5_ws: [n tile][chunk][tap][piece][lane] x 16 bytes."""
    return cdiv(Cout, 32) * cdiv(Cin, BS_CK) * 3 * ks * ks * 1024


def ws_bytes(C, K, ks=3):
    """clhip_conv3x3_bs_ws / clhip_conv5x5_bs_ws: the larger of the two directions' images."""
    return max(image_bytes(C, K, ks), image_bytes(K, C, ks))


def index_ok(Cin, Cout, H, W, ks=3):
    """clhip_internal_bs_index_ok: the int byte offsets of bs_conv_body inside the images of one block.  Input side: xoff * 4 plus
    (cb + e * plane_in) * 4 reach NI * Cin * H * W * 4 (NI = 2 images per block in the 8-wide geometry); output side:
    ((k * H + oh) * W + ow) * 4 reaches Cout * H * W * 4; the weight image: its size, which the descriptor clips at 2^31 - 1."""
    ni = 2 if (ks == 3 and W <= 8) else 1
    return ni * Cin * H * W < 1 << 29 and Cout * H * W < 1 << 29 and image_bytes(Cin, Cout, ks) <= LIMIT


def entry_ok(kind, N, C, K, H, W):
    Cin, Cout = kernel_view(kind, C, K)
    return N > 0 and bs_ok(Cin, Cout, H, W)


def geometry(W):
    """bs_launch: (RW, RH, NI) of BsGeo<32,4,1,2,2,1>, <16,8,1,2,2,1>, <8,8,2,2,2,1>."""
    return (32, 4, 1) if W > 16 else (16, 8, 1) if W > 8 else (8, 8, 2)


GB = (32, 2, 1)                      # BsGeo<32,2,1,2,1,1>: the second geometry of the mixed grid
POOL_WIDTH = {(32, 4, 1): 16, (16, 8, 1): 8, (8, 8, 2): 4, GB: 8}      # PW = RGW / 2 codes per (channel, pooled row) of a wave's region


def blocks(geo, N, Cout, H, W):
    """bs_launch_geo: pixel blocks rounded up to the 8-block XCD group, times the 64-channel groups."""
    RW, RH, NI = geo
    npb = cdiv(W, RW) * cdiv(H, RH) * cdiv(N, NI)
    return npb, cdiv(npb, 8) * 8 * cdiv(Cout, BS_BN)


def mixed_split(N, Cout, H, W, slots=256 * 3):
    """bs_launch_mixed32: NA, the images that go out as GA tiles, or None when the one-geometry launch runs.  slots: 256 CUs x
    bs_blocks_per_cu<GA> = 3 (2 x 6 planes of 3744 bytes = 44 928 bytes of LDS per block) for every instance."""
    if not (W > 16 and not ((H | W) & 1)):
        return None
    kts = cdiv(Cout, BS_BN)
    per_img_a = cdiv(W, 32) * cdiv(H, 4)
    total = per_img_a * N * kts
    rounds = total // slots
    rem = total - rounds * slots
    if rounds < 1 or rem == 0 or 2 * rem > slots:
        return None
    na = rounds * slots // (per_img_a * kts)
    if na < 1 or na >= N or na % 8:
        return None
    return na


def epilogue(H, W, pool=False, codes_on_dword=True):
    """The store form of bs_conv_body: 'scalar' (odd maps, lane by lane), 'float4' (the fast path through LDS: W % 4 == 0, and with
    pooling OW % 4 == 0 and the codes on a 4-byte boundary), else 'float2' (2x2 windows as two float2) / 'window' (pooled: one
    value and one code byte per lane and window)."""
    if (H | W) & 1:
        assert not pool
        return "scalar"
    if W % 4 == 0 and (not pool or ((W // 2) % 4 == 0 and codes_on_dword)):
        return "float4"
    return "window" if pool else "float2"


def code_store(geo, H, W, codes_on_dword=True):
    """How the pooled forward stores its codes: 'byte' in the window epilogue, else 'vector' when every region row is whole
    (OW % PW == 0) or 'vector+tail' when the last region of a row goes out byte by byte."""
    if epilogue(H, W, True, codes_on_dword) != "float4":
        return "byte"
    return "vector" if (W // 2) % POOL_WIDTH[geo] == 0 else "vector+tail"


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad_ok(C, K, H, W):
    """clhip_internal_bs_wgrad_ok: the 16-pixel kernel."""
    return (C >= 64 and C % 64 == 0 and K >= 64 and K % 64 == 0 and W >= 16 and W % 16 == 0 and H >= 1
            and C * H * W * 4 < LIMIT and K * H * W * 4 < LIMIT)


def wgrad_rows(N, H, W):
    return N * (W // 16) * H


def wgrad_splits(N, C, K, H, W):
    return min(max(256 // ((K // 64) * (C // 64)), 1), wgrad_rows(N, H, W))


def wgrad_ws(N, C, K, H, W):
    return wgrad_splits(N, C, K, H, W) * (9 * K * C + K) * 4 if N > 0 and wgrad_ok(C, K, H, W) else 0


def wgrad_shares(N, H, W, splits):
    """Per slab the list of (n, strip, ya, yb, ys, ye): dy rows [ya, yb) of column (n, strip), x rows ys .. ye, as bs_wgrad_kernel
    cuts the (image, strip, row) list."""
    rows, strips = wgrad_rows(N, H, W), W // 16
    per, extra = rows // splits, rows % splits
    out = []
    for split in range(splits):
        rr = split * per + min(split, extra)
        r_end = rr + per + (1 if split < extra else 0)
        segs = []
        while rr < r_end:
            ya, colid = rr % H, rr // H
            yb = min(H, ya + (r_end - rr))
            segs.append((colid // strips, colid % strips, ya, yb, ya - 1 if ya > 0 else 0, yb if yb < H else H - 1))
            rr += yb - ya
        out.append(segs)
    return out


def bsk3_ok(N, C, K, H, W):
    """bsk_ok<3>: the tap-split kernel."""
    return (N >= 1 and C >= 32 and C % 32 == 0 and K >= 32 and K % 32 == 0 and W >= 8 and H >= 1
            and N * C * H * W * 4 < LIMIT and N * K * H * W * 4 < LIMIT)


def bsk3_splits(N, C, K, H, W):
    types = (K // 32) * (C // 32) * 3
    return max(1, min(2048 // types, N * cdiv(W, 16) * H))


def bsk3_ws(N, C, K, H, W):
    return bsk3_splits(N, C, K, H, W) * (9 * K * C + K) * 4 if bsk3_ok(N, C, K, H, W) else 0


def wg_route(N, C, K, H, W, codes=False):
    """clhip_conv3x3_bs_bwd_weight: 'strip' (bs_wgrad_kernel), 'tap' (bs_wgradk_kernel<3,1>) or ENOTSUP."""
    if not codes and N > 0 and not wgrad_ok(C, K, H, W):
        return "tap" if bsk3_ok(N, C, K, H, W) else ENOTSUP
    if N <= 0 or not wgrad_ok(C, K, H, W) or (codes and (H | W) & 1):
        return ENOTSUP
    return "strip"


def wg_ws(N, C, K, H, W):
    """clhip_conv3x3_bs_bwd_weight_ws."""
    return wgrad_ws(N, C, K, H, W) or bsk3_ws(N, C, K, H, W)


def wg_splits(N, C, K, H, W):
    return wgrad_splits(N, C, K, H, W) if wgrad_ok(C, K, H, W) else bsk3_splits(N, C, K, H, W)


# ------------------------------------------------------------------------------------------------ the cases
# forward: shape, geometry, (pixel blocks, grid), epilogue plain / pooled (None: odd map), code store, what the row is there for
FWD_CASES = [
    ((3, 32, 64, 4, 4), (8, 8, 2), (2, 8), "float4", "window", "byte", "odd N: the second image of the last pair is missing; two chunks; half of every tile idle"),
    ((1, 32, 64, 5, 7), (8, 8, 2), (1, 8), "scalar", None, None, "odd map in the 8-wide geometry, one image of the pair"),
    ((2, 64, 64, 8, 8), (8, 8, 2), (1, 8), "float4", "float4", "vector", "the full tile: b32 code stores"),
    ((3, 64, 64, 12, 8), (8, 8, 2), (4, 8), "float4", "float4", "vector", "H > 8: two row tiles, the second half full; odd N"),
    ((2, 32, 64, 6, 6), (8, 8, 2), (1, 8), "float2", "window", "byte", "W % 4 == 2"),
    ((1, 32, 64, 4, 9), (16, 8, 1), (1, 8), "scalar", None, None, "W just above the switch, odd"),
    ((2, 64, 64, 8, 12), (16, 8, 1), (2, 8), "float4", "window", "byte", "OW = 6: fast plain, window pooled"),
    ((1, 64, 128, 10, 16), (16, 8, 1), (2, 16), "float4", "float4", "vector", "two row tiles, two channel groups: b64 code stores"),
    ((1, 32, 64, 13, 13), (16, 8, 1), (2, 8), "scalar", None, None, "AlexNet's small map"),
    ((1, 64, 64, 6, 14), (16, 8, 1), (1, 8), "float2", "window", "byte", ""),
    ((1, 32, 64, 4, 17), (32, 4, 1), (1, 8), "scalar", None, None, "W just above the switch, odd"),
    ((2, 64, 64, 6, 20), (32, 4, 1), (4, 8), "float4", "window", "byte", "OW = 10"),
    ((1, 96, 64, 5, 33), (32, 4, 1), (4, 8), "scalar", None, None, "six chunks; the second column tile has one column"),
    ((1, 64, 192, 8, 36), (32, 4, 1), (4, 24), "float4", "window", "byte", "three channel groups; OW = 18"),
    ((1, 64, 64, 6, 18), (32, 4, 1), (2, 8), "float2", "window", "byte", "W % 4 == 2 in the 32-wide geometry (not a row of the issue)"),
    ((1, 32, 64, 4, 24), (32, 4, 1), (1, 8), "float4", "float4", "vector+tail", "OW = 12 < PW = 16: every code row goes out byte by byte"),
    ((2, 64, 64, 8, 32), (32, 4, 1), (4, 8), "float4", "float4", "vector", "the bench model's map width: b128 code stores"),
    ((1, 32, 64, 4, 40), (32, 4, 1), (2, 8), "float4", "float4", "vector+tail", "OW = 20: one b128 store and a four-byte tail in the same code row (not a row of the issue)"),
]
# backward-data: the rows above with C % 64 == 0 and K % 32 == 0 (K >= 32), plus three of its own
BWD_EXTRA = [
    ((2, 64, 32, 8, 8), (8, 8, 2), (1, 8), "float4", "K = 32: two chunks"),
    ((1, 128, 32, 6, 20), (32, 4, 1), (2, 16), "float4", "two channel groups of dx"),
    ((1, 64, 96, 7, 27), (32, 4, 1), (2, 8), "scalar", "K = 96, AlexNet's width"),
]


def bwd_cases():
    rows = [(s, g, None, e) for s, g, _, e, _, _, _ in FWD_CASES if s[1] % 64 == 0 and s[2] % 32 == 0]
    return rows + [(s, g, b, e) for s, g, b, e, _ in BWD_EXTRA]


# the mixed grid: (N, C, K, H, W) of the forward (backward-data: C and K swapped), NA or None
MIXED_CASES = [
    ((192, 32, 128, 6, 24), None, "768 GA blocks: rem == 0"),
    ((200, 32, 128, 6, 24), 192, "800 blocks = one round + 32: images 192 .. 199 as GB tiles"),
    ((296, 32, 128, 6, 24), None, "1184 blocks: rem = 416, 2 rem > 768"),
    # table only (tensors above 32 MB)
    ((392, 32, 128, 6, 24), 384, "two rounds + 32"),
    ((100, 64, 64, 32, 32), 96, "the bench model's layer 2 at half its batch: 8 blocks per image"),
    ((195, 32, 128, 6, 24), 192, "780 blocks: rem = 12, the three last images as GB tiles"),
]

# 16-pixel weight gradient: shape, splits, codes run too, what the row is there for
WG_CASES = [
    ((1, 64, 64, 1, 16), 1, False, "H = 1: one row, ys = ye = 0"),
    ((1, 64, 64, 2, 16), 2, True, "H = 2, one-row shares"),
    ((1, 64, 64, 3, 32), 6, False, "H = 3, two strips"),
    ((2, 64, 64, 2, 16), 4, True, "the minimum with codes and two images"),
    ((2, 64, 64, 5, 32), 20, False, "rows = 20 < 256: every share one row"),
    ((3, 128, 64, 7, 16), 21, False, "two tiles, rows = 21 < 128: one-row shares across images"),
    ((5, 64, 128, 6, 48), 90, True, "rows = 90 < 128: one-row shares across strips and images"),
    ((3, 256, 256, 7, 16), 16, False, "rows = 21 over 16 slabs: per = 1, extra = 5; share 3 = rows 6 .. 7 crosses images 0 | 1"),
    ((3, 128, 256, 5, 48), 32, False, "rows = 45 over 32 slabs: per = 1, extra = 13; share 2 crosses strips, share 7 images"),
    ((2, 256, 256, 2, 16), 4, True, "16 tiles: 16 slabs wanted, 4 rows there"),
    ((70, 64, 64, 4, 16), 256, True, "rows = 280 > 256: 24 shares of two rows, 232 of one"),
]
WG_TABLE_ONLY = [((1, 1024, 1088, 1, 16), 1, "272 tiles > 256: one slab")]

# tap-split 3x3: shape, splits
BSK3_CASES = [
    ((1, 32, 32, 1, 8), 1, "both minima"),
    ((2, 32, 64, 3, 9), 6, ""),
    ((1, 64, 32, 13, 13), 13, "AlexNet's small map"),
    ((2, 32, 32, 4, 16), 8, "whole strips, but C % 64 != 0"),
    ((1, 64, 96, 6, 24), 12, "two strips, the second half masked"),
    ((3, 32, 32, 5, 17), 30, "the second strip has one column"),
]

# index width: (Cin, Cout, H, W, ks) just inside / just beyond each limit of index_ok
INDEX_INSIDE = [(32, 64, 2048, 4095, 3), (128, 64, 1024, 4095, 3), (64, 64, (1 << 19) - 1, 8, 3), (64, 64, 1 << 19, 9, 3),
                (4672, 8512, 4, 4, 3),              # 266 n tiles x 292 chunks x 27 KB = 2 147 475 456 bytes
                (14912, 960, 4, 9, 5)]              # 30 x 932 x 75 KB = 2 147 328 000 bytes
INDEX_BEYOND = [(32, 64, 2048, 4096, 3), (128, 64, 1024, 4096, 3), (64, 64, 1 << 19, 8, 3), (4672, 8576, 4, 4, 3), (4704, 8512, 4, 4, 3),
                (14912, 1024, 4, 9, 5)]


def check_tables():
    for s, geo, blk, ep, ep_pool, cs, _ in FWD_CASES:
        N, C, K, H, W = s
        assert entry_ok("fwd", *s) and index_ok(C, K, H, W), s
        assert geometry(W) == geo and blocks(geo, N, K, H, W) == blk, (s, geometry(W), blocks(geo, N, K, H, W))
        assert epilogue(H, W) == ep, (s, epilogue(H, W))
        if (H | W) & 1:
            assert ep_pool is None and cs is None
        else:
            assert epilogue(H, W, True) == ep_pool and code_store(geo, H, W) == cs, (s, epilogue(H, W, True), code_store(geo, H, W))
            assert epilogue(H, W, True, codes_on_dword=False) == "window" and code_store(geo, H, W, False) == "byte"
        assert mixed_split(N, K, H, W) is None, s
    for s, geo, blk, ep in bwd_cases():
        N, C, K, H, W = s
        assert entry_ok("bwd_data", *s) and index_ok(K, C, H, W), s
        assert geometry(W) == geo and epilogue(H, W) == ep, s
        assert blk is None or blocks(geo, N, C, H, W) == blk, (s, blocks(geo, N, C, H, W))
        assert mixed_split(N, C, H, W) is None, s
    assert len(bwd_cases()) >= 8
    geos = {g for _, g, _, _, _, _, _ in FWD_CASES}
    assert geos == {(32, 4, 1), (16, 8, 1), (8, 8, 2)}
    assert {(g, e) for _, g, _, e, _, _, _ in FWD_CASES} >= {(g, e) for g in geos for e in ("scalar", "float4", "float2")}
    assert {(g, c) for _, g, _, _, _, c, _ in FWD_CASES if c} >= {(g, c) for g in geos for c in ("byte", "vector")} | {((32, 4, 1), "vector+tail")}
    # the tail of the code store is not reachable in the two narrow geometries: there W <= 16, and OW % 4 == 0 leaves OW == PW
    for W in range(4, 17, 2):
        assert code_store(geometry(W), 4, W) in ("byte", "vector")
    for s, na, _ in MIXED_CASES:
        N, C, K, H, W = s
        assert mixed_split(N, K, H, W) == na, (s, mixed_split(N, K, H, W))
    # na % 8: 64 blocks per image (512 out-channels at 32 x 32) fill one round with 12 images, two rounds with 24
    assert mixed_split(13, 512, 32, 32) is None and mixed_split(25, 512, 32, 32) == 24
    assert mixed_split(200, 128, 7, 24) is None and mixed_split(200, 128, 6, 16) is None            # odd maps, W <= 16
    for s, _, _ in MIXED_CASES[:3]:
        N, C, K, H, W = s
        assert max(N * C * H * W, N * K * H * W) * 4 < 32 << 20, s
        assert epilogue(H, W, True) == "float4" and code_store(GB, H, W) == "vector+tail" and code_store((32, 4, 1), H, W) == "vector+tail"
    for s, splits, codes, _ in WG_CASES:
        N, C, K, H, W = s
        assert wg_route(*s) == "strip" and wgrad_splits(*s) == splits, (s, wgrad_splits(*s))
        assert wg_route(*s, codes=True) == ("strip" if not (H | W) & 1 else ENOTSUP)
        assert not codes or not (H | W) & 1
        assert wg_ws(*s) == splits * (9 * K * C + K) * 4
        sh = wgrad_shares(N, H, W, splits)
        rows = sorted((n, sx, y) for segs in sh for n, sx, ya, yb, _, _ in segs for y in range(ya, yb))
        assert rows == sorted((n, sx, y) for n in range(N) for sx in range(W // 16) for y in range(H)), s      # every dy row in exactly one share
        assert all(0 <= ys <= ye < H and ys in (ya, ya - 1) and ye in (yb, yb - 1) for segs in sh for _, _, ya, yb, ys, ye in segs)
    for s, splits, _ in WG_TABLE_ONLY:
        assert wg_route(*s) == "strip" and wgrad_splits(*s) == splits
    sh = wgrad_shares(3, 7, 16, 16)
    assert sh[3] == [(0, 0, 6, 7, 5, 6), (1, 0, 0, 1, 0, 1)] and sh[5] == [(1, 0, 3, 4, 2, 4)] and len(sh[0][0]) == 6
    sh = wgrad_shares(3, 5, 48, 32)
    assert sh[2] == [(0, 0, 4, 5, 3, 4), (0, 1, 0, 1, 0, 1)] and sh[7] == [(0, 2, 4, 5, 3, 4), (1, 0, 0, 1, 0, 1)]
    sh = wgrad_shares(70, 4, 16, 256)
    assert sum(1 for segs in sh if sum(yb - ya for _, _, ya, yb, _, _ in segs) == 2) == 24
    assert wgrad_shares(1, 1, 16, 1) == [[(0, 0, 0, 1, 0, 0)]]
    for s, splits, _ in BSK3_CASES:
        N, C, K, H, W = s
        assert wg_route(*s) == "tap" and bsk3_splits(*s) == splits and wg_route(*s, codes=True) == ENOTSUP, (s, bsk3_splits(*s))
        assert wg_ws(*s) == splits * (9 * K * C + K) * 4 and wg_splits(*s) == splits
    assert wg_route(1, 32, 48, 4, 16) == ENOTSUP and wg_route(1, 64, 64, 4, 7) == ENOTSUP and wg_route(0, 64, 64, 4, 16) == ENOTSUP
    for row in INDEX_INSIDE:
        assert bs_ok(*row[:4]) and index_ok(*row), row
    for row in INDEX_BEYOND:
        assert bs_ok(*row[:4]) and not index_ok(*row), row
