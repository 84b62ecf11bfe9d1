"""Argument checks of the bf16-split 3x3 entry points — clhip_conv3x3_bs_ws / _bs_fwd / _bs_bwd_data (csrc/bsconv.hip),
clhip_conv3x3_bs_bwd_weight_ws / _bs_bwd_weight (csrc/bswgrad.hip, csrc/bswgrad5.hip) — and the index-width refusal the 5x5 pair
clhip_conv5x5_bs_fwd / _bs_bwd_data shares with them, against the rules restated in bs_dispatch.py.  Runs without a GPU: the pointers
are dummies that are never dereferenced, because every call asserted on here is turned down before it launches anything.  (A call
that does reach a launch answers with a HIP error number on a machine without a GPU, never with a CLHIP_E* code; the tests that use
this to tell `refused` from `launched` run only where there is no GPU.)

Order of the checks, read from the code and written into include/clhip.h:
  clhip_conv3x3_bs_fwd / _bs_bwd_data   N <= 0 or a shape outside clhip_internal_bs_ok (of the kernel's view: C, K forward; K, C
                                        backward-data) -> ENOTSUP; a NULL x / w / y (dy / w / dx) or ws, or ws_bytes below the
                                        weight image -> EINVAL (no ENOSPC here); a size beyond clhip_internal_bs_index_ok -> EINVAL;
                                        codes on an odd map -> ENOTSUP; then the weight-image launch.
  clhip_conv3x3_bs_bwd_weight           without codes and outside the 16-pixel kernel's shapes: the tap-split kernel's checks
                                        (shape -> ENOTSUP, NULL -> EINVAL, workspace -> ENOSPC); otherwise N <= 0, the shape, codes on
                                        an odd map -> ENOTSUP; NULL x / dy / dw / ws -> EINVAL; workspace -> ENOSPC.

Found with this file (each assertion named fails on the parent library):
  * refusal fixed: clhip_conv3x3_bs_fwd / _bs_bwd_data / clhip_conv5x5_bs_fwd / _bs_bwd_data took every size inside
    clhip_internal_bs_ok, so bs_conv_body formed int byte offsets past 2^31 inside one image and the descriptor of a weight image
    above 2 GB was clipped (test_index_width_limits on the parent: the calls beyond the limits reach the launch);
  * refusal fixed: clhip_internal_bs_ok took Cout = 0 and negative multiples of 64 (`Cout % 64 == 0`), which the entry points then
    answered with EINVAL from the weight-image job instead of ENOTSUP (test_domain_refusals)."""
import ctypes as C

import bs_dispatch as d

EINVAL, ENOSPC, ENOTSUP = -1, -2, -3
CODES = (EINVAL, ENOSPC, ENOTSUP)
BIG = 1 << 40
OK = (2, 64, 64, 8, 16)                                # N, C, K, H, W: taken by all three entry points (16-pixel weight gradient)


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(128)
    p = (C.addressof(buf) + 15) & ~15
    return L, p, buf


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _entries(L):
    """name -> call(q, shape, idx, ws, ws_bytes); q: the four float pointers in the entry's own order (the third of fwd / bwd and
    the fourth of wg are optional: bias, relu_src, db)."""
    def fwd(q, s, idx, ws, n):
        return L.clhip_conv3x3_bs_fwd(q[0], q[1], q[2], q[3], idx, *s, 1, ws, n, None)

    def bwd(q, s, idx, ws, n):
        return L.clhip_conv3x3_bs_bwd_data(q[0], idx, q[1], q[2], q[3], *s, ws, n, None)

    def wg(q, s, idx, ws, n):
        return L.clhip_conv3x3_bs_bwd_weight(q[0], q[1], idx, q[2], q[3], *s, ws, n, None)
    return dict(fwd=fwd, bwd=bwd, wg=wg)


REQUIRED = dict(fwd=(0, 1, 3), bwd=(0, 1, 3), wg=(0, 1, 2))


def test_tables_follow_from_the_rules():
    d.check_tables()


def test_workspace_sizes_are_the_restated_ones():
    L, p, _keep = _setup()
    chans = [1, 3, 16, 31, 32, 33, 48, 63, 64, 65, 96, 128, 160, 192, 255, 256, 320, 512, 1000, 1024, 4672, 8512]
    n = 0
    for Cc in chans:
        for K in chans:
            assert L.clhip_conv3x3_bs_ws(Cc, K) == d.ws_bytes(Cc, K) > 0, (Cc, K)
            assert L.clhip_conv5x5_bs_ws(Cc, K) == d.ws_bytes(Cc, K, 5) > 0, (Cc, K)
            n += 1
    assert d.ws_bytes(32, 64) == 2 * 2 * 27 * 1024 and d.ws_bytes(64, 32) == d.ws_bytes(32, 64)      # by hand: 2 n tiles x 2 chunks
    assert d.ws_bytes(32, 192) == max(6 * 2, 1 * 12) * 27 * 1024
    shapes = [(N, Cc, K, H, W) for N in (0, 1, 2, 3, 70, 200) for Cc in (0, 16, 32, 48, 64, 96, 128, 256, 1024) for K in (0, 16, 32, 64, 96, 128, 256, 1088)
              for H in (0, 1, 2, 3, 5, 13, 32) for W in (4, 7, 8, 9, 13, 16, 17, 24, 32, 48)]
    shapes += [s for s, _, _, _ in d.WG_CASES] + [s for s, _, _ in d.WG_TABLE_ONLY + d.BSK3_CASES]
    assert len(shapes) + n > 2000
    zero = 0
    for s in shapes:
        want = d.wg_ws(*s)
        assert L.clhip_conv3x3_bs_bwd_weight_ws(*s) == want, s
        refused = d.wg_route(*s) == ENOTSUP
        assert (want == 0) == refused, s
        zero += refused
    assert 0 < zero < len(shapes)
    # the 2 GB limits of the two weight-gradient kernels: per image on the 16-pixel kernel, the whole tensor on the tap-split one
    assert d.wg_ws(4096, 64, 64, 128, 1024) > 0 and L.clhip_conv3x3_bs_bwd_weight_ws(4096, 64, 64, 128, 1024) == d.wg_ws(4096, 64, 64, 128, 1024)
    for s in ((1, 64, 64, 8192, 1024), (1, 32, 32, 16384, 1024), (64, 32, 32, 512, 520)):
        assert d.wg_ws(*s) == 0 and L.clhip_conv3x3_bs_bwd_weight_ws(*s) == 0, s


def test_null_pointers_batch_and_workspace():
    L, p, _keep = _setup()
    E = _entries(L)
    full = [p, p, p, p]
    need = dict(fwd=d.image_bytes(64, 64), bwd=d.image_bytes(64, 64), wg=d.wg_ws(*OK))
    assert need["wg"] == L.clhip_conv3x3_bs_bwd_weight_ws(*OK) > 0
    for name, call in E.items():
        short = ENOSPC if name == "wg" else EINVAL                   # forward / backward-data have no ENOSPC (clhip.h)
        for null in REQUIRED[name]:
            q = list(full)
            q[null] = None
            assert call(q, OK, None, p, BIG) == EINVAL, (name, null)
            assert call(q, OK, None, p, need[name] - 1) == EINVAL, (name, null)       # NULL is judged before the workspace size
        assert call(full, OK, None, None, BIG) == EINVAL, name                         # ws is required
        for nbytes in (need[name] - 1, 0):
            assert call(full, OK, None, p, nbytes) == short, (name, nbytes)
            assert call(full, OK, p, p, nbytes) == short, (name, nbytes)
        for N in (0, -1):
            s = (N,) + OK[1:]
            assert call(full, s, None, p, BIG) == ENOTSUP, (name, s)
            assert call([None] * 4, s, None, None, 0) == ENOTSUP, (name, s)            # ... before anything else
        assert L.clhip_conv3x3_bs_bwd_weight_ws(0, *OK[1:]) == 0 and L.clhip_conv3x3_bs_bwd_weight_ws(-1, *OK[1:]) == 0
    # the tap-split kernel's own checks, reached without codes at W = 8
    s = (2, 64, 64, 8, 8)
    assert d.wg_route(*s) == "tap"
    for null in REQUIRED["wg"]:
        q = list(full)
        q[null] = None
        assert E["wg"](q, s, None, p, BIG) == EINVAL
    assert E["wg"](full, s, None, p, d.wg_ws(*s) - 1) == ENOSPC and E["wg"](full, s, None, None, BIG) == EINVAL


def test_domain_refusals():
    """Channels, H and W outside the domain: ENOTSUP, before the NULL checks."""
    L, p, _keep = _setup()
    E = _entries(L)
    full = [p, p, p, p]
    N, Cc, K, H, W = OK
    bad = dict(
        fwd=[(N, c, K, H, W) for c in (0, 16, 48, -32)] + [(N, Cc, k, H, W) for k in (0, 32, 96, -64)],
        bwd=[(N, c, K, H, W) for c in (0, 32, 96, -64)] + [(N, Cc, k, H, W) for k in (0, 16, 48, -32)],
        wg=[(N, c, K, H, W) for c in (0, 16, 48, -64)] + [(N, Cc, k, H, W) for k in (0, 16, 48, -64)] + [(N, Cc, K, 0, W), (N, Cc, K, -1, W), (N, Cc, K, H, 7), (N, Cc, K, H, 0)])
    for name in ("fwd", "bwd"):
        bad[name] += [(N, Cc, K, h, W) for h in (3, 0, -4)] + [(N, Cc, K, H, w) for w in (3, 0, -4)]
    for name, rows in bad.items():
        for s in rows:
            if name == "wg":
                assert d.wg_route(*s) == ENOTSUP and L.clhip_conv3x3_bs_bwd_weight_ws(*s) == 0, s
            else:
                assert not d.entry_ok("fwd" if name == "fwd" else "bwd_data", *s), s
            assert E[name](full, s, None, p, BIG) == ENOTSUP, (name, s)
            assert E[name]([None] * 4, s, None, None, 0) == ENOTSUP, (name, s)
    # the two directions see the channels the other way round: 32 out-channels are a shape of backward-data only, 96 of neither ...
    assert E["fwd"](full, (2, 64, 32, 8, 8), None, p, BIG) == ENOTSUP and E["bwd"](full, (2, 32, 64, 8, 8), None, p, BIG) == ENOTSUP
    # ... and the weight gradient takes 32-channel multiples on the tap-split kernel, where W >= 8 suffices (answers: its workspace check)
    for s in ((2, 32, 96, 8, 8), (1, 96, 32, 1, 13)):
        assert d.wg_route(*s) == "tap" and E["wg"](full, s, None, p, 0) == ENOSPC, s


def test_codes_refusals():
    L, p, _keep = _setup()
    E = _entries(L)
    full = [p, p, p, p]
    for H, W in ((5, 16), (8, 17), (7, 33)):
        s = (2, 64, 64, H, W)
        need = d.image_bytes(64, 64)
        for name in ("fwd", "bwd"):
            assert E[name](full, s, p, p, need) == ENOTSUP, (name, s)               # codes on an odd map, before the weight launch
            assert E[name](full, s, p, p, need - 1) == EINVAL, (name, s)            # ... behind the workspace and NULL checks
            q = list(full)
            q[0] = None
            assert E[name](q, s, p, p, need) == EINVAL, (name, s)
    # weight gradient: codes on an odd map and codes with a shape the 16-pixel kernel does not take, before NULL and workspace
    for s in ((2, 64, 64, 5, 16), (2, 64, 64, 4, 17), (2, 64, 64, 8, 8), (2, 32, 64, 8, 16), (2, 64, 96, 8, 16), (1, 64, 64, 13, 13), (2, 64, 64, 8, 24)):
        assert d.wg_route(*s, codes=True) == ENOTSUP, s
        assert E["wg"](full, s, p, p, BIG) == ENOTSUP, s
        assert E["wg"]([None] * 4, s, p, None, 0) == ENOTSUP, s
    # with the same shapes and no codes the tap-split kernel answers (here: its workspace check), where its rules take the shape
    for s in ((2, 64, 64, 5, 16), (2, 64, 64, 8, 8), (2, 32, 64, 8, 16), (1, 64, 64, 13, 13)):
        route = d.wg_route(*s)
        assert route in ("tap", "strip") and E["wg"](full, s, None, p, 0) == ENOSPC, s
    assert d.wg_route(2, 64, 64, 4, 16, codes=True) == "strip" and E["wg"](full, (2, 64, 64, 4, 16), p, p, 0) == ENOSPC


def _layer(kind, Cin, Cout):
    return (Cin, Cout) if kind == "fwd" else (Cout, Cin)


def test_index_width_limits():
    """Sizes beyond what the int offsets of bs_conv_body carry inside the images of one block (bs_dispatch.index_ok, derived there):
    CLHIP_EINVAL from the 3x3 and the 5x5 pair before the weight-image launch — on the parent these calls reached the launch.  Just
    inside each limit, and for batches whose whole tensors are far above 2 GB (the descriptors are re-based at the block's first
    image in size_t, the plain-pointer accesses use size_t offsets), the call goes through to the launch."""
    L, p, _keep = _setup()
    full = [p, p, p, p]

    def call(kind, ks, N, Cin, Cout, H, W, idx=None):
        Cc, K = _layer(kind, Cin, Cout)
        if ks == 3 and kind == "fwd":
            return L.clhip_conv3x3_bs_fwd(p, p, p, p, idx, N, Cc, K, H, W, 1, p, BIG, None)
        if ks == 3:
            return L.clhip_conv3x3_bs_bwd_data(p, idx, p, p, p, N, Cc, K, H, W, p, BIG, None)
        if kind == "fwd":
            return L.clhip_conv5x5_bs_fwd(p, p, p, p, N, Cc, K, H, W, 1, p, BIG, None)
        return L.clhip_conv5x5_bs_bwd_data(p, p, p, p, N, Cc, K, H, W, p, BIG, None)

    for Cin, Cout, H, W, ks in d.INDEX_BEYOND:
        assert d.bs_ok(Cin, Cout, H, W) and not d.index_ok(Cin, Cout, H, W, ks)
        for kind in ("fwd", "bwd_data"):
            for N in (1, 3):
                assert call(kind, ks, N, Cin, Cout, H, W) == EINVAL, (kind, N, Cin, Cout, H, W, ks)
            if ks == 3 and not (H | W) & 1:
                assert call(kind, ks, 1, Cin, Cout, H, W, idx=p) == EINVAL
    # what is beyond for 3x3 because two images share a block (W <= 8) is inside for the one-image geometries
    assert d.index_ok(64, 64, 1 << 19, 9) and not d.index_ok(64, 64, 1 << 19, 8) and d.index_ok(64, 64, 1 << 19, 9, 5)
    # codes on an odd map stay ENOTSUP inside the limits and become EINVAL beyond them (the order of clhip.h)
    assert call("fwd", 3, 1, 32, 64, 2047, 4096, idx=p) == ENOTSUP and call("fwd", 3, 1, 32, 64, 2049, 4096, idx=p) == EINVAL
    if _no_gpu():
        for Cin, Cout, H, W, ks in d.INDEX_INSIDE:
            assert d.index_ok(Cin, Cout, H, W, ks)
            for kind in ("fwd", "bwd_data"):
                assert call(kind, ks, 1, Cin, Cout, H, W) not in CODES, (kind, Cin, Cout, H, W, ks)
        # 2^20 images of 64 x 32 x 32: 256 GB tensors, 2^23 blocks
        for kind in ("fwd", "bwd_data"):
            assert call(kind, 3, 1 << 20, 64, 64, 32, 32) not in CODES
            assert call(kind, 5, 1 << 20, 64, 64, 32, 32) not in CODES
        # accepted calls do not change: the table's smallest shapes go through to the launch
        x = (C.c_float * 65536)()
        q = C.addressof(x)
        assert L.clhip_conv3x3_bs_fwd(q, q, q, q, None, 1, 32, 64, 4, 4, 1, q, d.ws_bytes(32, 64), None) not in CODES
        assert L.clhip_conv3x3_bs_bwd_data(q, None, q, q, q, 1, 64, 32, 4, 4, q, d.ws_bytes(64, 32), None) not in CODES
