"""The un-pooling staging maps of the bf16-split backward-data kernel and of the 16-tile Winograd kernel (csrc/stage_map.hpp, read
through the host entry clhip_internal_stage_map, a test hook that include/clhip.h does not declare: the kernels and the entry call
the same functions) against the per-pixel rules they replace, stated here in numpy.  Runs without a GPU.  First the bf16-split kernel; the Winograd kernel's rule is stated at its test below.

The old rule: an item is (halo pixel, k half).  Halo pixel (ni, hy, hx) of the tile at (image n0, row y0, column x0) is image pixel
(gy, gx) = (y0 + hy - 1, x0 + hx - 1) of image n0 + ni; inside the image it loads channel 8 h (and the 7 behind it) of pooled element
(gy >> 1, gx >> 1) with the code byte and keeps the value where code == 2 (gy & 1) + (gx & 1); outside it stages zeros.  It writes slot
h * PLANE_SLOTS + ((ni // IPR) * HR + hy) * P + (ni % IPR) * HW + hx.

The new map writes per (window of a halo row, k half).  For every pixel block of the launch: every slot of the halo image gets exactly
the (source, position) of the old rule, slots written more than once (windows cut by the halo edge, the spare threads of the round) get
identical content, slots outside the image get zeros, and no pooled element is loaded more than twice per block and chunk."""
import ctypes as C

import numpy as np
import pytest

# geo -> (RW, RH, NI): the BsGeo instances of csrc/bsconv.hip (3 x 3 taps: halo 1)
GEOS = {0: (32, 4, 1), 1: (32, 2, 1), 2: (16, 8, 1), 3: (8, 8, 2)}
SIZES = [(8, 8), (16, 16), (32, 32), (8, 64)]
N, CIN = 3, 32                      # N = 3: the two-image geometry's last block holds one image and one past the batch


def _hook():
    """clhip_internal_stage_map (csrc/stage_map.hpp): exported by the library, bound here by name"""
    from clsurvey_amd import _lib
    fn = _lib.lib().clhip_internal_stage_map
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)] * 3 + [C.c_int]
    return fn


def _geo(geo):
    RW, RH, NI = GEOS[geo]
    IPR = 2 if RW == 8 else 1
    HW, HR = RW + 2, RH + 2
    P = (IPR * HW + 7) // 16 * 16 + 8
    ROWS = (NI // IPR) * HR
    PLANE_SLOTS = (ROWS - 1) * P + IPR * HW
    return RW, RH, NI, IPR, HW, HR, P, PLANE_SLOTS


def _old_rule(geo, H, W, block):
    """{slot: (src, pos)} of the per-pixel staging; src = -1: zeros (pos is then irrelevant and left out)"""
    RW, RH, NI, IPR, HW, HR, P, PLANE_SLOTS = _geo(geo)
    tiles_x, tiles_y = -(-W // RW), -(-H // RH)
    tx, ty, grp = block % tiles_x, (block // tiles_x) % tiles_y, block // (tiles_x * tiles_y)
    n0, y0, x0 = grp * NI, ty * RH, tx * RW
    plane = (H // 2) * (W // 2)
    want = {}
    for h in range(2):
        for ni in range(NI):
            for hy in range(HR):
                for hx in range(HW):
                    gy, gx, n = y0 + hy - 1, x0 + hx - 1, n0 + ni
                    slot = h * PLANE_SLOTS + ((ni // IPR) * HR + hy) * P + (ni % IPR) * HW + hx
                    if n < N and 0 <= gy < H and 0 <= gx < W:
                        want[slot] = ((n * CIN + 8 * h) * plane + (gy >> 1) * (W // 2) + (gx >> 1), 2 * (gy & 1) + (gx & 1))
                    else:
                        want[slot] = (-1, None)
    return want


def _map(geo, H, W, block):
    cap = 4096
    src, pos, slot = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    n = _hook()(0, geo, N, CIN, H, W, block, src, pos, slot, cap)
    assert 0 < n <= cap and n % 512 == 0, n          # whole rounds of 256 items, two writes each
    return np.array(src[:n]), np.array(pos[:n]), np.array(slot[:n])


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("geo", sorted(GEOS))
def test_every_block_stages_the_old_halo_image(geo, hw):
    H, W = hw
    RW, RH, NI = GEOS[geo]
    npb = _hook()(0, geo, N, CIN, H, W, -1, None, None, None, 0)
    assert npb == -(-W // RW) * -(-H // RH) * -(-N // NI)
    for block in range(npb):               # first, interior and last tile of every image, the ragged last image group
        want = _old_rule(geo, H, W, block)
        src, pos, slot = _map(geo, H, W, block)
        assert len(src) == 512             # one round on every geometry (the per-pixel rule took two)
        got = {}
        for s, p, q in zip(src.tolist(), pos.tolist(), slot.tolist()):
            content = (s, p) if s >= 0 else (-1, None)
            assert got.setdefault(q, content) == content, (block, q)          # written twice: identical content
        # the spare threads of the round: zeros into the padding behind the halo pixels of an LDS row of the first plane
        _, _, _, IPR, HW, HR, P, PLANE_SLOTS = _geo(geo)
        for q in sorted(set(got) - set(want)):
            assert got.pop(q) == (-1, None) and 0 <= q < PLANE_SLOTS and q % P >= IPR * HW, (block, q)
        assert got == want, block
        assert np.array_equal(src[0::2], src[1::2])      # one load per item: its two writes share it
        items = 2 * NI * HR * (RW // 2 + 2)
        assert (src[2 * items:] == -1).all()             # the spare threads load nothing
        loads = src[0::2]
        _, counts = np.unique(loads[loads >= 0], return_counts=True)
        assert counts.size == 0 or counts.max() <= 2, block


def test_refusals():
    buf = (C.c_int * 8)()
    assert _hook()(3, 0, N, CIN, 8, 8, -1, None, None, None, 0) == -3          # kernels 0 (bf16-split), 1 (wino_conv16g), 2 (plain wino_conv16) have maps
    assert _hook()(1, 2, N, CIN, 8, 8, -1, None, None, None, 0) == -3
    assert _hook()(1, 0, N, 12, 16, 16, -1, None, None, None, 0) == -1         # the Winograd path: whole 8-channel chunks, 16 or more
    assert _hook()(0, 4, N, CIN, 8, 8, -1, None, None, None, 0) == -3
    assert _hook()(0, 0, N, CIN, 7, 8, -1, None, None, None, 0) == -1          # un-pooling wants even maps
    assert _hook()(0, 0, N, 24, 8, 8, -1, None, None, None, 0) == -1           # whole 16-channel chunks
    assert _hook()(0, 0, N, CIN, 8, 8, 6, buf, buf, buf, 8) == -1              # 6 blocks: 0 .. 5
    assert _hook()(0, 0, N, CIN, 8, 8, 0, None, buf, buf, 8) == -1
    assert _hook()(0, 0, N, CIN, 8, 8, 0, buf, buf, buf, 8) == 512             # the arrays take the first `cap`


# ---------------------------------------------------------------------------------------------------- wino_conv16g_body (kernel 1)
# geo -> (TC, TR, EROWS): wino_conv16g_kernel<8, 2, 4> (even maps >= 16 wide) and <4, 4, 4> (two whole 8 x 8 images per block)
W_GEOS = {0: (8, 2, 4), 1: (4, 4, 4)}
W_CIN = 16


def _w_old_rule(geo, H, W, block):
    """The per-element staging: element e of the chunk buffer [4 channels][entity][PRE][PW] is image pixel (h, w) =
    (2 EROWS g - 1 + row, w0 - 1 + col) of entity v0 + ent = (image, row group g); inside the image it loads pooled element
    (h >> 1, w >> 1) of its channel and keeps it where code == 2 (h & 1) + (w & 1)."""
    TC, TR, ER = W_GEOS[geo]
    NE, PW, PRE = 2 * TR // ER, 2 * TC + 2, 2 * ER + 2
    PLANE = NE * PRE * PW
    tiles_w, tiles_h = -(-(W // 2) // TC), -(-(H // 2) // ER)
    bw, v0 = block % tiles_w, (block // tiles_w) * NE
    w0 = bw * 2 * TC
    plane = (H // 2) * (W // 2)
    want = {}
    for e in range(4 * PLANE):
        cl, rem = divmod(e, PLANE)
        rr, col = divmod(rem, PW)
        ent, row = divmod(rr, PRE)
        nn, g = divmod(v0 + ent, tiles_h)
        h, w = g * 2 * ER - 1 + row, w0 - 1 + col
        if nn < N and 0 <= h < H and 0 <= w < W:
            want[e] = ((nn * W_CIN + cl) * plane + (h >> 1) * (W // 2) + (w >> 1), 2 * (h & 1) + (w & 1))
        else:
            want[e] = (-1, None)
    return want


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("geo", sorted(W_GEOS))
def test_wino16g_every_block_stages_the_old_halo_planes(geo, hw):
    H, W = hw
    TC, TR, ER = W_GEOS[geo]
    NE = 2 * TR // ER
    npb = _hook()(1, geo, N, W_CIN, H, W, -1, None, None, None, 0)
    assert npb == -(-(N * -(-(H // 2) // ER)) // NE) * -(-(W // 2) // TC)
    cap = 4096
    src, pos, slot = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    for block in range(npb):
        want = _w_old_rule(geo, H, W, block)
        n = _hook()(1, geo, N, W_CIN, H, W, block, src, pos, slot, cap)
        assert n == 4 * 4 * NE * (ER + 2) * (TC + 2) <= cap          # four writes per pooled window of every (channel, entity) plane
        got = {}
        for s, p, q in zip(src[:n], pos[:n], slot[:n]):
            content = (s, p) if s >= 0 else (-1, None)
            assert got.setdefault(q, content) == content, (block, q)
        assert got == want, block
        loads = np.array(src[:n])[0::4]
        assert np.array_equal(np.repeat(loads, 4), np.array(src[:n]))
        _, counts = np.unique(loads[loads >= 0], return_counts=True)
        # every pooled value once per block and chunk; twice where the block's two entities are neighbouring row groups of ONE image and
        # share a halo row (<4, 4, 4> off the 8 x 8 maps it is launched for)
        assert counts.size == 0 or counts.max() <= (1 if NE == 1 or (H, W) == (8, 8) else 2), block


# ---------------------------------------------------------------------------------------------------- plain wino_conv16_body (kernel 2)
@pytest.mark.parametrize("kt2", [1, 2])
def test_wino16_plain_every_block_stages_the_old_halo_planes(kt2):
    """The per-element rule: element e of the chunk buffer [8 channels][KT2 images][10][10] is pixel (row - 1, col - 1) of image
    n0 + nb; inside the 8 x 8 image (and the batch) it holds that element of the input tensor, else zero.  The new staging writes the
    interior as float4s of image rows and the ring once: every slot exactly once, ring and images past the batch zero, every input
    element loaded once, every float4 inside one image row."""
    cin = 16
    plane = kt2 * 100
    npb = _hook()(2, kt2 - 1, N, cin, 8, 8, -1, None, None, None, 0)
    assert npb == -(-N // kt2)
    cap = 4096
    src, pos, slot = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    for block in range(npb):
        want = {}
        for e in range(8 * plane):
            cl, rem = divmod(e, plane)
            rr, col = divmod(rem, 10)
            nb, row = divmod(rr, 10)
            n, h, w = block * kt2 + nb, row - 1, col - 1
            want[e] = ((n * cin + cl) * 64 + h * 8 + w) if n < N and 0 <= h < 8 and 0 <= w < 8 else -1
        n = _hook()(2, kt2 - 1, N, cin, 8, 8, block, src, pos, slot, cap)
        assert n == 8 * plane <= cap                       # every slot of the buffer written exactly once
        got = dict(zip(slot[:n], src[:n]))
        assert len(got) == n and got == want, block
        items = np.array(src[:8 * kt2 * 64]).reshape(-1, 4)
        live = items[items[:, 0] >= 0]
        assert (np.diff(live, axis=1) == 1).all() and (live[:, 0] % 4 == 0).all()      # contiguous, whole float4s of the tensor
        sl = np.array(slot[:8 * kt2 * 64]).reshape(-1, 4)
        assert (np.diff(sl, axis=1) == 1).all()
    assert _hook()(2, 2, N, cin, 8, 8, -1, None, None, None, 0) == -3
    assert _hook()(2, 0, N, cin, 16, 16, -1, None, None, None, 0) == -1
