"""Kernel-level parity of the bf16-split 3x3 kernels: clhip_conv3x3_bs_fwd / clhip_conv3x3_bs_bwd_data (every 3x3 instantiation of
bs_conv_body in csrc/bsconv.hip: BsGeo<8,8,2>, <16,8,1>, <32,4,1>, the mixed grid with <32,2,1>, with and without fused pooling /
un-pooling, and the weight image they build) and clhip_conv3x3_bs_bwd_weight (bs_wgrad_kernel<false> / <true> / <true, bytes> of
csrc/bswgrad.hip and bs_wgradk_kernel<3,1> of csrc/bswgrad5.hip with their slab reduction), called with raw pointers into one
kernel_parity.Arena (codes: a ByteArena), each against the fp64 convolution of the same float32 inputs.

Dispatch.  bs_dispatch.py restates the rules and carries the rows (FWD_CASES, bwd_cases(), MIXED_CASES, WG_CASES, BSK3_CASES) with
what each is there for, and the two corrections of the issue's rows (the per-byte tail of the code store; shares with extra != 0).

Accuracy rule, per element: |device - fp64| <= ((Kd + splits + 3) * 2^-24 + 2^-26) * S[e] + 2^-24 * |bias| — the rule of
test_gpu_conv5x5_bs_kernels.py unchanged; Kd = 9 C forward, 9 K backward-data, N*H*W weight gradient; splits = the restated slab
count (1 for forward / backward-data).  db: the any-order bound (N*H*W + splits + 3) * 2^-24 * sum|dy|.

Alignment of the arg-max codes (read before the byte-address runs were sent).  The pooled fast epilogue stores a region row of codes
with one raw_buffer_store_b128 / _b64 / _b32 at a dword multiple of pool_idx, bs_wgrad_kernel<true> loads four codes with one
raw_buffer_load_b32 at a dword multiple of idx; backward-data reads codes with byte loads.  Dword-aligned multi-dword buffer
accesses are what the float operands one and two floats off a 16-byte boundary already exercise; nothing in the sources or the
kernel guides defines a dword access at a byte address, so the entry points were re-routed, nothing refused: with codes off a
4-byte boundary the forward takes the window epilogue (byte stores) and the weight gradient the instance that loads four bytes.
test_*_codes_at_byte_addresses check the re-route (same bits as aligned at the odd default address, at an even non-dword one and
at a dword one that is not 16-byte aligned; no byte outside the tensor).

Measured on one MI355X (one run with -s; device error / bound, float32-CPU error / bound, worst over the variants of a test):
  conv_every_row / float_operands_off_a_16_byte_boundary, forward: 0.001 - 0.005 / 0.001 - 0.010 over the 18 rows (worst (1,32,64,13,13),
    (1,32,64,4,17), (1,32,64,4,24), (1,32,64,4,40): 0.005; C = 32 has the smallest Kd); backward-data: 0.001 - 0.007 / 0.000 - 0.006 over the 12 rows
    (worst (1,128,32,6,20): 0.007).  backward_data_unpools, plain dy: 0.001 - 0.006 / 0.001 - 0.006.
    mixed_grid, images [0:2], [190:194], [N-2:N]: forward 0.004 - 0.006 / 0.010, backward-data 0.004 - 0.005 / 0.008; the plain forward of
    the slices that the pooled variant is held against 0.004 - 0.006 / 0.010, the explicitly un-pooled backward-data of the slices that
    the with-codes variant is held against 0.005 - 0.009 / 0.011.
  weight_gradient_every_row        dw              db error / (2^-24 sum|dy|) | its bound N*H*W + splits + 3
  (1,64,64,1,16)               0.054 / 0.160   0.918 | 20
  (1,64,64,2,16)               0.035 / 0.106   0.709 | 37
  (1,64,64,3,32)               0.008 / 0.036   0.275 | 105
  (2,64,64,2,16)               0.017 / 0.048   0.433 | 71
  (2,64,64,5,32)               0.001 / 0.012   0.226 | 343
  (3,128,64,7,16)              0.001 / 0.013   0.158 | 360
  (5,64,128,6,48)              0.000 / 0.003   0.128 | 1533
  (3,256,256,7,16)             0.002 / 0.014   0.191 | 355
  (3,128,256,5,48)             0.000 / 0.007   0.154 | 755
  (2,256,256,2,16)             0.021 / 0.064   0.572 | 71
  (70,64,64,4,16)              0.000 / 0.001   0.061 | 4739
  (1,32,32,1,8)                0.098 / 0.249   0.679 | 12         tap-split kernel from here on
  (2,32,64,3,9)                0.016 / 0.048   0.328 | 63
  (1,64,32,13,13)              0.003 / 0.018   0.245 | 185
  (2,32,32,4,16)               0.005 / 0.014   0.309 | 139
  (1,64,96,6,24)               0.004 / 0.024   0.281 | 159
  (3,32,32,5,17)               0.002 / 0.005   0.186 | 288
  weight_gradient_unpools (explicitly un-pooled dy): (1,64,64,2,16) 0.057 / 0.071, db 1.507 | 37; (2,64,64,2,16) 0.027 / 0.048, 0.768 | 71;
    (5,64,128,6,48) 0.000 / 0.003, 0.139 | 1533; (2,256,256,2,16) 0.034 / 0.058, 0.874 | 71; (70,64,64,4,16) 0.000 / 0.001, 0.106 | 4739
  error_is_that_of_an_fp32_chain, all-positive operands, error / S in units of 2^-24 (max, rms): bf16-split | f32 sibling
  (3,64,64,12,8) fwd            9.09  2.09 | 22.8  5.63       ratio 0.40 0.37
  (1,32,64,13,13) fwd           5.59  1.56 | 16.6  4.06       ratio 0.34 0.38
  (1,96,64,5,33) fwd            9.92  2.43 | 24.2  6.57       ratio 0.41 0.37
  (2,64,32,8,8) bwd_data        5.70  1.50 | 16.1  3.92       ratio 0.35 0.38
  (2,64,64,8,12) bwd_data       8.25  2.12 | 22.3  5.60       ratio 0.37 0.38
  (1,64,96,7,27) bwd_data       11.1  2.43 | 27.9  6.73       ratio 0.40 0.36
  (5,64,128,6,48) bwd_weight    0.96  0.38 | 1.27  0.41       ratio 0.76 0.93     (16-pixel kernel)
  (1,64,32,13,13) bwd_weight    1.56  0.43 | 2.21  0.60       ratio 0.71 0.71     (tap-split kernel)
  Run time on the MI355X: 205 tests in 7.1 s (siblings: 3.5 s and 10.6 s); slowest 0.47 s
  (weight_gradient_operands_off_a_16_byte_boundary[3x128x256x5x48]: nine launches with 38 MB of slabs each), 0.22 s for the first test
  (library load), at most 0.39 s for any other.

Mutation check, run once against scratch copies of csrc/bsconv.hip, bs_weight.hpp and bswgrad.hip (one run of this file per mutant with
CLHIP_LIB on the mutant library; arithmetic, selections and comparisons only, no address, load / store bound or barrier changed; not
part of the repository; run on the 188 tests the file had before the weight-gradient alignment test took every row, (1,32,64,4,40) was
added and the pooled / with-codes variants of mixed_grid got their slice checks — additions only).  Failing tests of this file per mutant:
  mask `ms.x >= 0.f` (float4 epilogue)          21: conv_every_row x9 and float_operands_off.. x9 (backward-data, W % 4 == 0), mixed_grid x3 (bwd_data)
  mask `m0.x >= 0.f` (float2 epilogue)           4: conv_every_row and float_operands_off.. at (1,64,64,6,14), (1,64,64,6,18) backward-data
  mask `mask_src[o] >= 0.f` (scalar epilogue)    2: the same two tests at (1,64,96,7,27) backward-data (the only odd backward-data row)
  dead test `!(mx >= 0.f)`, fast epilogue       10: fused_pooling[relu] x5 (the five float4 rows), pooled_forward_codes_at_byte_addresses x5
  dead test `!(mx >= 0.f)`, window epilogue     17: fused_pooling[relu] x12 (seven window rows; the five float4 rows through their b[0] = 0.5 run at the odd
                                                    default code address, which is the re-route), pooled_forward_codes_at_byte_addresses x5
  arg-max `y01 >= mx`, fast epilogue             5: fused_pooling[no relu] on the five float4 rows (ties of the zero out-channel: code 1)
  arg-max `y01 >= mx`, window epilogue          19: fused_pooling
  `pos` from gx only (un-pooling staging)       11: backward_data_unpools, every row
  `a2` / `a2 + 1u` swapped in split_d            5: weight_gradient_unpools, every row
  `ok = y >= ya && y <= yb` in load_d           22: weight_gradient_every_row x11 (the 16-pixel rows), _unpools x5, _shares x5, error_is.. x1
  `ye = H - 1` always                            0: EQUIVALENT in values.  ye bounds the WORK of a share: the x rows behind yb meet dy rows outside
                                                    [ya, yb), which load_d reads as zeros, so every extra product adds +0 to a sum that started at
                                                    +0; only the run time grows, which no result shows.
  one piece product dropped in row_taps (a2 b0)  6: weight_gradient_every_row at H = 1, 2, _unpools x3, error_is.. (5,64,128,6,48)
  one piece product dropped in BS_TERM (a2 b0)   2: error_is_that_of_an_fp32_chain (1,32,64,13,13) fwd and (2,64,32,8,8) bwd_data — the 2^-17 |a b|
                                                    it loses per term lies inside the any-order bound of (a) at Kd = 288, so only the comparison
                                                    with the f32 sibling sees it, and only at the two C = 32 rows
  staging into chunk parity `c & 1`            144: everything forward / backward-data
  180-degree flip removed (backward-data image) 43: every backward-data accuracy test, weight_image_is_an_exact_split x2, mixed_grid x3
  `na % 8` dropped from the mixed rule          not built: EQUIVALENT in values (an output's sum does not depend on its tile, so only the block order
                                                    changes), and no row here has na % 8 != 0 (bs_dispatch.check_tables: 13 images of 512 x 32 x 32)."""
import pytest
import torch

import bs_dispatch as bd
import conv_parity as cp
from conv_parity import BYTE_OUT, U, WS_SLACK, accuracy, check_ws, operands, reference, run_call, unit_errors
from kernel_parity import ConvRef, all_bits, bitwise_equal

pytestmark = pytest.mark.gpu

DROPPED = 2.0 ** -26          # the three piece products a1 b2, a2 b1, a2 b2 the kernels leave out (header of bsconv.hip)
DEAD = 4


def full(s5):
    N, Cc, K, H, W = s5
    return (N, Cc, H, W, K, 3, 3, 1, 1)


def _sid(s5):
    return "x".join(str(v) for v in s5)


def ws_floats_of(kind, s5):
    N, Cc, K, H, W = s5
    if kind == "bwd_weight":
        return bd.wg_ws(*s5) // 4
    return bd.image_bytes(*bd.kernel_view(kind, Cc, K)) // 4


def run3(L, kind, s5, x=None, w=None, dy=None, bias=None, relu=0, relu_src=None, pool=False, codes=None, want_db=True, mis=None, mis_by=1,
         bshift=None, ws_finite=True):
    """One raw call.  fwd: pool=True asks for pooled values + codes.  bwd_data / bwd_weight: codes != None: dy is the pooled gradient.
    ws_finite=False: the weight gradient's slabs may hold a planted NaN (every element must still have been written)."""
    N, Cc, K, H, W = s5
    need = ws_floats_of(kind, s5)
    bins, bouts = (), ()
    if kind == "fwd":
        n_out = N * K * (H // 2) * (W // 2) if pool else N * K * H * W
        ins, outs = [("x", x), ("w", w), ("b", bias)], [("out", n_out)]
        bouts = [("codes", n_out if pool else None)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv3x3_bs_fwd(p["x"], p["w"], p["b"], p["out"], p["codes"], N, Cc, K, H, W, int(relu), ws, nbytes, stream)
    elif kind == "bwd_data":
        ins, outs = [("dy", dy), ("w", w), ("src", relu_src)], [("out", N * Cc * H * W)]
        bins = [("codes", codes)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv3x3_bs_bwd_data(p["dy"], p["codes"], p["w"], p["src"], p["out"], N, Cc, K, H, W, ws, nbytes, stream)
    else:
        ins, outs = [("x", x), ("dy", dy)], [("out", K * Cc * 9), ("db", K if want_db else None)]
        bins = [("codes", codes)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv3x3_bs_bwd_weight(p["x"], p["dy"], p["codes"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    r = run_call(call, ins, outs, ws_floats=need + WS_SLACK, ws_bytes=4 * need, mis=mis, mis_by=mis_by, bins=bins, bouts=bouts, bshift=bshift)
    assert r.rc == 0 and r.clean, "%s %s: rc %d, gaps, guards or inputs changed: %s" % (kind, s5, r.rc, not r.clean)
    check_ws(r.ws, need, "%s %s" % (kind, s5), finite=(kind == "bwd_weight" and ws_finite))
    return r


def run_f32(L, kind, s5, x, w, dy):
    """The f32 sibling on the same data: clhip_conv3x3_fwd / _bwd_data / _bwd_weight."""
    N, Cc, K, H, W = s5
    need = L.clhip_conv3x3_bwd_weight_ws(*s5) // 4 if kind == "bwd_weight" else 0
    if kind == "fwd":
        ins, outs = [("x", x), ("w", w)], [("out", N * K * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv3x3_fwd(p["x"], p["w"], None, p["out"], N, Cc, K, H, W, 0, stream)
    elif kind == "bwd_data":
        ins, outs = [("dy", dy), ("w", w)], [("out", N * Cc * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv3x3_bwd_data(p["dy"], p["w"], None, p["out"], N, Cc, K, H, W, stream)
    else:
        ins, outs = [("x", x), ("dy", dy)], [("out", K * Cc * 9), ("db", K)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv3x3_bwd_weight(p["x"], p["dy"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    r = run_call(call, ins, outs, ws_floats=need)
    assert r.rc == 0 and r.clean
    return r


def unpool(dyp, codes):
    """max_pool2d backward followed by ReLU backward: [N][K][OH][OW] + codes 0..4 -> [N][K][2 OH][2 OW]."""
    N, K, OH, OW = dyp.shape
    out = torch.zeros((N, K, OH, 2, OW, 2))
    for q in range(4):
        out[:, :, :, q >> 1, :, q & 1] = torch.where(codes == q, dyp, torch.zeros(()))
    return out.reshape(N, K, 2 * OH, 2 * OW)


def pooled_inputs(s5, seed=5):
    N, Cc, K, H, W = s5
    gen = torch.Generator().manual_seed(seed + 31 * N + 7 * K + H + 3 * W)
    dyp = torch.randn((N, K, H // 2, W // 2), generator=gen)
    codes = torch.randint(0, 5, (N, K, H // 2, W // 2), generator=gen, dtype=torch.uint8)
    return dyp, codes


def first_max(v):
    """v [N][K][H][W] -> (2x2 maxima, position of the first maximum in ATen's scan order): bs_conv_body's own `>` chain."""
    N, K, H, W = v.shape
    q = v.view(N, K, H // 2, 2, W // 2, 2)
    mx, am = q[:, :, :, 0, :, 0].clone(), torch.zeros((N, K, H // 2, W // 2), dtype=torch.uint8)
    for i in (1, 2, 3):
        c = q[:, :, :, i >> 1, :, i & 1]
        gt = c > mx
        mx, am = torch.where(gt, c, mx), torch.where(gt, torch.full_like(am, i), am)
    return mx, am


# --------------------------------------------------------------------------------------------- a, b, e: forward / backward-data
def check_conv(case, L, kind, s5, only=None, mis=None, mis_by=1):
    N, Cc, K, H, W = s5
    shape = full(s5)
    x, w, dy = operands(shape)
    want, cpu, Sabs = cp.ref_of(kind, reference(shape))
    bias, src = cp.epilogue_inputs(shape)
    Kd = 9 * (Cc if kind == "fwd" else K)
    if kind == "fwd":
        vs = [("bias-relu", dict(bias=bias, relu=1), dict(bias=bias, relu=True)), ("bias", dict(bias=bias), dict(bias=bias)), ("plain", {}, {})]
    else:
        vs = [("relu_src", dict(relu_src=src), dict(mask_src=src)), ("plain", {}, {})]
    outs = {}
    for name, kw, acc in vs:
        if only is not None and name != only:
            continue
        r = run3(L, kind, s5, x=x, w=w, dy=dy, mis=mis, mis_by=mis_by, **kw)
        accuracy(case, name, r.out["out"], want, cpu, Sabs, Kd, 1, extra=DROPPED, **acc)
        outs[name] = r.out["out"]
    if only is not None:
        return outs
    if kind == "fwd":
        assert torch.equal(outs["bias-relu"], outs["bias"].clamp(min=0)), "relu is not max(v, 0) of the same v"
        assert all_bits(outs["bias-relu"].view(N, K, H, W)[:, 0], 0), "zero weights, b = -0.0, ReLU: the output must be exactly +0.0"
        assert bool((outs["plain"].view(N, K, H, W)[:, 0] == 0).all())
    else:
        on = src.reshape(-1) > 0
        assert bitwise_equal(outs["relu_src"][on], outs["plain"][on]), "relu_src > 0 must pass the value through unchanged"
        assert all_bits(outs["relu_src"][~on], 0), "relu_src of 0.0, -0.0, a negative denormal or NaN must give exactly +0.0"
    return outs


FWD = [r[0] for r in bd.FWD_CASES]
BWD = [r[0] for r in bd.bwd_cases()]
CONV = [(s, "fwd") for s in FWD] + [(s, "bwd_data") for s in BWD]


@pytest.mark.parametrize("s5,kind", CONV, ids=["%s-%s" % (_sid(s), k) for s, k in CONV])
def test_bs3_conv_every_row(request, s5, kind):
    """Per element against fp64, bias = NULL and relu_src = NULL included, exact epilogue bits, exactly the weight image written."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    assert L.clhip_conv3x3_bs_ws(Cc, K) == bd.ws_bytes(Cc, K) and bd.entry_ok(kind, *s5)
    check_conv(request.node.name, L, kind, s5)


EVEN = [s for s in FWD if not (s[3] | s[4]) & 1]


@pytest.mark.parametrize("s5", EVEN, ids=[_sid(s) for s in EVEN])
@pytest.mark.parametrize("relu", [0, 1])
def test_bs3_fused_pooling(s5, relu):
    """Pooled values = the 2x2 maxima of the same entry point's un-pooled output, codes = the first maximum of those sums (exact ties
    on the zero out-channel: code 0, or 4 under ReLU with b = -0.0; a positive bias there: code 0), 4 exactly where ReLU leaves no
    positive maximum; all bit for bit; no byte outside the code tensor (run3: ByteArena gaps)."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    x, w, dy = operands(full(s5))
    bias, _ = cp.epilogue_inputs(full(s5))
    y = run3(L, "fwd", s5, x=x, w=w, bias=bias, relu=relu).out["out"].view(N, K, H, W)
    r = run3(L, "fwd", s5, x=x, w=w, bias=bias, relu=relu, pool=True, bshift={"codes": 0})
    mx, am = first_max(y)
    if relu:
        am = torch.where(mx > 0, am, torch.full_like(am, DEAD))
    assert bitwise_equal(r.out["out"].view(mx.shape), mx), "pooled values are not the maxima of the un-pooled output"
    got = r.out["codes"].view(am.shape)
    assert torch.equal(got, am), "codes: %d differ" % int((got != am).sum())
    assert bool((got[:, 0] == (DEAD if relu else 0)).all()) and bool((got[:, 1:] != DEAD).any())
    if relu:
        assert bool((got[:, 1:] == DEAD).any()) or H * W * N < 64, "no dead window in the random channels"
        b2 = bias.clone()
        b2[0] = 0.5
        r2 = run3(L, "fwd", s5, x=x, w=w, bias=b2, relu=1, pool=True)
        assert bool((r2.out["codes"].view(am.shape)[:, 0] == 0).all()) and bool((r2.out["out"].view(mx.shape)[:, 0] == 0.5).all())
        assert torch.equal(r2.out["codes"].view(am.shape)[:, 1:], got[:, 1:])


EVEN_BWD = [s for s in BWD if not (s[3] | s[4]) & 1]


def _unpool_case(L, kind, s5, **kw):
    """Pooled dy + codes against the same entry point on the explicitly un-pooled gradient; returns (pooled run, plain run, dy_u)."""
    x, w, _ = operands(full(s5))
    dyp, codes = pooled_inputs(s5)
    dyu = unpool(dyp, codes)
    a = run3(L, kind, s5, x=x, w=w, dy=dyp, codes=codes, **kw)
    b = run3(L, kind, s5, x=x, w=w, dy=dyu)
    assert bitwise_equal(a.out["out"], b.out["out"]), "%s %s: un-pooling in the kernel differs from the explicit gradient" % (kind, s5)
    return a, b, dyu, dyp, codes


@pytest.mark.parametrize("s5", EVEN_BWD, ids=[_sid(s) for s in EVEN_BWD])
def test_bs3_backward_data_unpools(request, s5):
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    x, w, _ = operands(full(s5))
    a, b, dyu, dyp, codes = _unpool_case(L, "bwd_data", s5)
    ref = ConvRef(x, w, dyu, 1, 1)
    accuracy(request.node.name, "plain dy", b.out["out"], ref.dx64, ref.dx32, ref.s_dx, 9 * K, 1, extra=DROPPED)
    # a NaN and an Inf under a dead code change nothing
    dead = (codes == DEAD).nonzero()
    assert len(dead) >= 2
    d2 = dyp.clone()
    d2[tuple(dead[0])], d2[tuple(dead[-1])] = float("nan"), float("inf")
    c = run3(L, "bwd_data", s5, w=w, dy=d2, codes=codes)
    assert bitwise_equal(c.out["out"], a.out["out"]), "a non-finite pooled gradient under a dead code reached dx"


# --------------------------------------------------------------------------------------------- weight gradient
WG = [r[0] for r in bd.WG_CASES] + [r[0] for r in bd.BSK3_CASES]
WG_CODES = [r[0] for r in bd.WG_CASES if r[2]]


def check_db(case, db, dy, Kd, splits):
    unit = U * dy.double().abs().sum((0, 2, 3))
    e = float(((db.double() - dy.double().sum((0, 2, 3))).abs() / unit).max())
    print("MEASURED|%s|db error / (2^-24 sum|dy|), bound %d|%.3f|-" % (case, Kd + splits + 3, e))
    assert bool(torch.isfinite(db).all()) and e <= Kd + splits + 3, "db: %.3f units, bound %d" % (e, Kd + splits + 3)


@pytest.mark.parametrize("s5", WG, ids=[_sid(s) for s in WG])
def test_bs3_weight_gradient_every_row(request, s5):
    """dw per element, db against the any-order bound, exactly splits * (9 K C + K) finite floats of workspace, two calls the same
    bits, db = NULL."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    splits = bd.wg_splits(*s5)
    assert L.clhip_conv3x3_bs_bwd_weight_ws(*s5) == bd.wg_ws(*s5) == splits * (9 * K * Cc + K) * 4
    x, w, dy = operands(full(s5))
    ref = reference(full(s5))
    r = run3(L, "bwd_weight", s5, x=x, dy=dy)
    accuracy(request.node.name, "dw", r.out["out"], ref.dw64, ref.dw32, ref.s_dw, N * H * W, splits, extra=DROPPED)
    check_db(request.node.name, r.out["db"], dy, N * H * W, splits)
    r2 = run3(L, "bwd_weight", s5, x=x, dy=dy)
    assert bitwise_equal(r.out["out"], r2.out["out"]) and bitwise_equal(r.out["db"], r2.out["db"]), "two calls differ"
    r3 = run3(L, "bwd_weight", s5, x=x, dy=dy, want_db=False)
    assert bitwise_equal(r.out["out"], r3.out["out"]), "dw must not depend on db being asked for"


@pytest.mark.parametrize("s5", WG_CODES, ids=[_sid(s) for s in WG_CODES])
def test_bs3_weight_gradient_unpools(request, s5):
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    splits = bd.wg_splits(*s5)
    x, w, _ = operands(full(s5))
    a, b, dyu, dyp, codes = _unpool_case(L, "bwd_weight", s5, bshift={"codes": 0})
    assert bitwise_equal(a.out["db"], b.out["db"])
    ref = ConvRef(x, w, dyu, 1, 1)
    accuracy(request.node.name, "plain dy", b.out["out"], ref.dw64, ref.dw32, ref.s_dw, N * H * W, splits, extra=DROPPED)
    check_db(request.node.name, b.out["db"], dyu, N * H * W, splits)
    dead = (codes == DEAD).nonzero()
    d2 = dyp.clone()
    d2[tuple(dead[0])], d2[tuple(dead[-1])] = float("nan"), float("inf")
    c = run3(L, "bwd_weight", s5, x=x, dy=d2, codes=codes, bshift={"codes": 0})
    assert bitwise_equal(c.out["out"], a.out["out"]) and bitwise_equal(c.out["db"], a.out["db"]), "a non-finite value under a dead code reached dw / db"


SHARE_ROWS = [(3, 128, 64, 7, 16), (5, 64, 128, 6, 48), (3, 256, 256, 7, 16), (3, 128, 256, 5, 48), (70, 64, 64, 4, 16)]


@pytest.mark.parametrize("s5", SHARE_ROWS, ids=[_sid(s) for s in SHARE_ROWS])
def test_bs3_weight_gradient_shares(s5):
    """One NaN in dy at the first and at the last row of a share (ya, yb - 1), on both sides of a strip and of an image boundary:
    exactly dW[k] at the taps whose x row lies inside the map and db[k] become non-finite; the taps of k whose x row lies outside
    the map (r = 0 for y = 0, r = 2 for y = H - 1: those x rows are not run) and every other out-channel keep the clean run's bits.
    A dy row that NO share consumed would leave dW[k] finite.  A NaN cannot show a row consumed TWICE (NaN + NaN is NaN): that is
    seen by the per-element bound of weight_gradient_every_row and _unpools alone, as the `y <= yb` mutant shows."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    splits = bd.wgrad_splits(*s5)
    shares = bd.wgrad_shares(N, H, W, splits)
    x, w, dy = operands(full(s5))
    clean = run3(L, "bwd_weight", s5, x=x, dy=dy)
    assert bool(torch.isfinite(clean.out["out"]).all())
    # first / last rows of shares at both ends of the list and on both sides of the first strip boundary and the first image boundary
    strips, rows = W // 16, bd.wgrad_rows(N, H, W)
    near = {0, rows - 1} | {b + o for b in (H, strips * H) for o in (-2, -1, 0, 1)}
    picks = sorted({(n, sx, y) for segs in shares for n, sx, ya, yb, _, _ in segs for y in (ya, yb - 1) if (n * strips + sx) * H + y in near})[:8]
    assert len(picks) >= 4 and {p[0] for p in picks} >= {0, 1}
    for i, (n, sx, y) in enumerate(picks):
        k = (7 + 13 * i) % K
        dy2 = dy.clone()
        dy2[n, k, y, 16 * sx + 5] = float("nan")
        r = run3(L, "bwd_weight", s5, x=x, dy=dy2, ws_finite=False)
        dw, dw0 = r.out["out"].view(K, Cc, 3, 3), clean.out["out"].view(K, Cc, 3, 3)
        others = torch.arange(K) != k
        assert bitwise_equal(dw[others], dw0[others]) and bitwise_equal(r.out["db"][others], clean.out["db"][others]), (n, sx, y)
        taps = [t for t in range(3) if 0 <= y + t - 1 < H]
        assert not bool(torch.isfinite(dw[k][:, taps]).any()) and not bool(torch.isfinite(r.out["db"][k])), \
            "dy row (image %d, strip %d, row %d) was not consumed" % (n, sx, y)
        outside = [t for t in range(3) if t not in taps]
        assert bitwise_equal(dw[k][:, outside], dw0[k][:, outside]), "a tap whose x row lies outside the map changed (row %d)" % y


# --------------------------------------------------------------------------------------------- e: the weight image
@pytest.mark.parametrize("Cc,K,kind", [(32, 192, "fwd"), (64, 96, "bwd_data"), (128, 32, "bwd_data")])
def test_bs3_weight_image_is_an_exact_split(Cc, K, kind):
    """test_gpu_bs.py::test_bs_weight_image_is_an_exact_split at two chunks x six n tiles and for backward-data images with C != K:
    the three bf16 pieces sum to the weight exactly, piece i is the bf16 rounding of what the pieces before it left, backward-data
    holds w[ci][ko] rotated by 180 degrees."""
    L = cp.product_lib()
    s5 = (1, Cc, K, 4, 8)
    x, w, dy = operands(full(s5))
    r = run3(L, kind, s5, x=x, w=w, dy=dy)
    Ci, Ko = bd.kernel_view(kind, Cc, K)
    n_nt, n_ch = Ko // 32, Ci // 16
    img = r.ws[:n_nt * n_ch * 27 * 256].contiguous().view(torch.int16).view(n_nt, n_ch, 9, 3, 2, 32, 8)      # [nt][chunk][tap][piece][kh][ko & 31][e]
    pieces = (img.to(torch.int32) << 16).view(torch.float32).double()
    val = pieces.permute(3, 0, 5, 1, 4, 6, 2).reshape(3, Ko, Ci, 9)
    wc = w.double()
    want = wc.reshape(K, Cc, 9) if kind == "fwd" else wc.reshape(K, Cc, 9).flip(2).permute(1, 0, 2)
    assert torch.equal(val.sum(0), want)
    assert torch.equal(val[0].float(), want.float().to(torch.bfloat16).float())
    assert torch.equal(val[1].float(), (want - val[0]).float().to(torch.bfloat16).float())
    assert torch.equal(val[2].float(), (want - val[0] - val[1]).float().to(torch.bfloat16).float())


# --------------------------------------------------------------------------------------------- f: off a 16-byte boundary
@pytest.mark.parametrize("s5,kind", CONV, ids=["%s-%s" % (_sid(s), k) for s, k in CONV])
def test_bs3_float_operands_off_a_16_byte_boundary(request, s5, kind):
    """x / w / bias / y (dy / w / mask / dx) in turn one and two floats past a 16-byte boundary: the aligned bits."""
    L = cp.product_lib()
    variant = "bias-relu" if kind == "fwd" else "relu_src"
    base = check_conv(request.node.name, L, kind, s5, only=variant)[variant]
    for name in (("out", "b", "x", "w") if kind == "fwd" else ("out", "src", "dy", "w")):
        for by in (1, 2):
            got = check_conv("%s[%s+%d]" % (request.node.name, name, by), L, kind, s5, only=variant, mis=name, mis_by=by)[variant]
            assert bitwise_equal(got, base), "%s %d floats off: the result changed" % (name, by)


@pytest.mark.parametrize("s5", WG, ids=[_sid(s) for s in WG])
def test_bs3_weight_gradient_operands_off_a_16_byte_boundary(s5):
    """Every row of both weight-gradient kernels: x, dy, dw and db in turn one and two floats past a 16-byte boundary — the aligned bits
    (run3: nothing outside the outputs and the promised workspace written, every slab element written)."""
    L = cp.product_lib()
    x, w, dy = operands(full(s5))
    base = run3(L, "bwd_weight", s5, x=x, dy=dy)
    for name in ("x", "dy", "out", "db"):
        for by in (1, 2):
            r = run3(L, "bwd_weight", s5, x=x, dy=dy, mis=name, mis_by=by)
            assert bitwise_equal(r.out["out"], base.out["out"]) and bitwise_equal(r.out["db"], base.out["db"]), "%s %d floats off" % (name, by)


BYTE_SHIFTS = (5, 2, 4)          # ByteArena's odd default; even, not a dword; a dword that is not 16-byte aligned


@pytest.mark.parametrize("s5", EVEN, ids=[_sid(s) for s in EVEN])
def test_bs3_pooled_forward_codes_at_byte_addresses(s5):
    """Off a 4-byte boundary the pooled forward takes the window epilogue (bs_dispatch.epilogue(.., codes_on_dword=False)): the
    same values and codes as with 16-byte aligned codes, no byte outside the tensor."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    assert bd.epilogue(H, W, True, codes_on_dword=False) == "window"
    x, w, dy = operands(full(s5))
    bias, _ = cp.epilogue_inputs(full(s5))
    base = run3(L, "fwd", s5, x=x, w=w, bias=bias, relu=1, pool=True, bshift={"codes": 0})
    assert not bool((base.out["codes"] == BYTE_OUT).any())
    for sh in BYTE_SHIFTS:
        r = run3(L, "fwd", s5, x=x, w=w, bias=bias, relu=1, pool=True, bshift={"codes": sh})
        assert bitwise_equal(r.out["out"], base.out["out"]) and torch.equal(r.out["codes"], base.out["codes"]), "codes %d bytes off" % sh


UNPOOLING = [("bwd_data", s) for s in EVEN_BWD] + [("bwd_weight", s) for s in WG_CODES]


@pytest.mark.parametrize("kind,s5", UNPOOLING, ids=["%s-%s" % (_sid(s), k) for k, s in UNPOOLING])
def test_bs3_unpooling_codes_at_byte_addresses(kind, s5):
    """Backward-data reads its codes byte by byte; the weight gradient loads four of them as one dword only on a 4-byte boundary and
    as four bytes otherwise (bs_wgrad_kernel<true, true>): the bits of the 16-byte aligned run."""
    L = cp.product_lib()
    x, w, _ = operands(full(s5))
    dyp, codes = pooled_inputs(s5)
    base = run3(L, kind, s5, x=x, w=w, dy=dyp, codes=codes, bshift={"codes": 0})
    for sh in BYTE_SHIFTS:
        r = run3(L, kind, s5, x=x, w=w, dy=dyp, codes=codes, bshift={"codes": sh})
        assert bitwise_equal(r.out["out"], base.out["out"]), "codes %d bytes off" % sh
        if kind == "bwd_weight":
            assert bitwise_equal(r.out["db"], base.out["db"])


# --------------------------------------------------------------------------------------------- g: the mixed grid
def big_operands(s5):
    """conv_parity.operands for batches of millions of elements (where a draw can be exactly zero: replaced by 1)."""
    N, Cc, K, H, W = s5
    gen = torch.Generator().manual_seed(977 * N + 17 * Cc + 5 * K + 7 * H + 3 * W)
    x, w, dy = torch.randn((N, Cc, H, W), generator=gen), torch.randn((K, Cc, 3, 3), generator=gen) * 0.05, torch.randn((N, K, H, W), generator=gen)
    x[x == 0], w[w == 0], dy[dy == 0] = 1.0, 0.05, 1.0
    w[0] = 0.0
    return x, w, dy


CHUNK = 96                      # 384 GA blocks: below one round, so a chunk always takes the one-geometry launch


@pytest.mark.parametrize("variant", ["fwd", "fwd-pool", "bwd_data", "bwd_data-codes"])
@pytest.mark.parametrize("row", bd.MIXED_CASES[:3], ids=[str(r[0][0]) for r in bd.MIXED_CASES[:3]])
def test_bs3_mixed_grid(request, row, variant):
    """Batches either side of each condition of bs_launch_mixed32.  Every image bit for bit the one-geometry launch on chunks of 96
    images.  Images [0:2], [190:194] (NA = 192 where the grid is mixed) and [N-2:N]: plain forward and backward-data per element
    against fp64; pooled forward = first_max() (+ the dead code) of the plain forward of the same slice, which is bounded against fp64
    here; backward-data with codes = the call on the explicitly un-pooled gradient of the slice, bounded against fp64 here."""
    L = cp.product_lib()
    (N, Cc, K, H, W), na, _ = row
    kind = "fwd" if variant.startswith("fwd") else "bwd_data"
    if kind == "bwd_data":
        Cc, K = K, Cc
    s5 = (N, Cc, K, H, W)
    Cin, Cout = bd.kernel_view(kind, Cc, K)
    assert bd.mixed_split(N, Cout, H, W) == na and bd.mixed_split(CHUNK, Cout, H, W) is None and bd.mixed_split(N % CHUNK or CHUNK, Cout, H, W) is None
    x, w, dy = big_operands(s5)
    bias, _ = cp.epilogue_inputs(full(s5))
    kw = {}
    if variant == "fwd-pool":
        kw = dict(pool=True)
    if variant == "bwd_data-codes":
        dy, codes = pooled_inputs(s5)
        kw = dict(codes=codes)
    if kind == "fwd":
        kw.update(bias=bias, relu=1)
    src = None
    if variant == "bwd_data":
        src = cp.epilogue_inputs(full(s5))[1]
        kw = dict(relu_src=src)

    def sl(t, a, e):
        return None if t is None else t[a:e].contiguous()
    whole = run3(L, kind, s5, x=x, w=w, dy=dy, **kw)
    per = whole.out["out"].numel() // N
    out = whole.out["out"].view(N, per)
    for a in range(0, N, CHUNK):
        e = min(a + CHUNK, N)
        kc = dict(kw)
        for key in ("codes", "relu_src"):
            if key in kc:
                kc[key] = sl(kc[key], a, e)
        c = run3(L, kind, (e - a, Cc, K, H, W), x=sl(x, a, e), w=w, dy=sl(dy, a, e), **kc)
        assert bitwise_equal(out[a:e], c.out["out"].view(e - a, per)), "images %d .. %d differ from the one-geometry launch" % (a, e)
        if variant == "fwd-pool":
            assert torch.equal(whole.out["codes"].view(N, per)[a:e], c.out["codes"].view(e - a, per))
    for a, e in ((0, 2), (190, min(194, N)), (N - 2, N)):
        what, ss = "images %d:%d" % (a, e), (e - a, Cc, K, H, W)
        if variant == "fwd-pool":
            ref = ConvRef(x[a:e], w, torch.zeros((e - a, K, H, W)), 1, 1)
            y = run3(L, "fwd", ss, x=sl(x, a, e), w=w, bias=bias, relu=1).out["out"]
            accuracy(request.node.name, what, y, ref.y64, ref.y32, ref.s_y, 9 * Cc, 1, extra=DROPPED, bias=bias, relu=True)
            mx, am = first_max(y.view(e - a, K, H, W))
            am = torch.where(mx > 0, am, torch.full_like(am, DEAD))
            assert bitwise_equal(out[a:e].reshape(mx.shape), mx), what + ": pooled values are not the maxima of the plain forward"
            assert torch.equal(whole.out["codes"].view(N, per)[a:e].reshape(am.shape), am), what + ": codes"
            continue
        if variant == "bwd_data-codes":
            dyu = unpool(dy[a:e], kw["codes"][a:e])
            ref = ConvRef(x[a:e], w, dyu, 1, 1)
            u = run3(L, "bwd_data", ss, w=w, dy=dyu).out["out"]
            accuracy(request.node.name, what, u, ref.dx64, ref.dx32, ref.s_dx, 9 * K, 1, extra=DROPPED)
            assert bitwise_equal(out[a:e].reshape(-1), u), what + ": un-pooling in the kernel differs from the explicit gradient"
            continue
        ref = ConvRef(x[a:e], w, dy[a:e], 1, 1)
        if kind == "fwd":
            accuracy(request.node.name, "images %d:%d" % (a, e), out[a:e], ref.y64, ref.y32, ref.s_y, 9 * Cc, 1, extra=DROPPED, bias=bias, relu=True)
        else:
            accuracy(request.node.name, "images %d:%d" % (a, e), out[a:e], ref.dx64, ref.dx32, ref.s_dx, 9 * K, 1, extra=DROPPED, mask_src=src[a:e])


# --------------------------------------------------------------------------------------------- i: locality and scale
LOCAL = [((3, 64, 64, 12, 8), "fwd"), ((3, 64, 64, 12, 8), "bwd_data"), ((1, 64, 128, 10, 16), "fwd"), ((1, 64, 96, 7, 27), "bwd_data"),
         ((2, 64, 64, 6, 20), "fwd")]


@pytest.mark.parametrize("s5,kind", LOCAL, ids=["%s-%s" % (_sid(s), k) for s, k in LOCAL])
def test_bs3_non_finite_stays_in_its_windows(s5, kind):
    """One NaN, then one Inf, in one pixel of x (dy) of the FIRST image (the left one of a pair in the 8-wide geometry): the outputs
    whose 3x3 window covers it are non-finite (the split turns Inf into NaN pieces: non-finite is what bsconv.hip promises), every
    other output keeps the clean run's bits."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    x, w, dy = operands(full(s5))
    clean = run3(L, kind, s5, x=x, w=w, dy=dy).out["out"]
    assert bool(torch.isfinite(clean).all())
    n_out = K if kind == "fwd" else Cc
    for val in (float("nan"), float("inf"), float("-inf")):
        for ph, pw in ((0, 0), (H // 2, W - 1), (H - 1, W // 2)):
            x2, dy2 = x.clone(), dy.clone()
            (x2 if kind == "fwd" else dy2)[0, (Cc if kind == "fwd" else K) - 1, ph, pw] = val
            hit = torch.zeros((N, 1, H, W), dtype=torch.bool)
            hit[0, 0, max(ph - 1, 0):ph + 2, max(pw - 1, 0):pw + 2] = True
            hit = hit.expand(N, n_out, H, W).reshape(-1)
            # (out-channel 0 has zero weights: 0 * NaN is NaN too, inside the window only)
            got = run3(L, kind, s5, x=x2, w=w, dy=dy2).out["out"]
            assert bitwise_equal(got[~hit], clean[~hit]), "%s leaked out of its windows" % val
            assert not bool(torch.isfinite(got[hit]).any()), "%s did not reach all of its windows" % val


SCALE = [((3, 32, 64, 4, 4), "fwd"), ((1, 64, 128, 10, 16), "fwd"), ((2, 64, 64, 6, 20), "fwd"), ((2, 64, 32, 8, 8), "bwd_data"), ((1, 64, 96, 7, 27), "bwd_data"),
         ((3, 128, 64, 7, 16), "bwd_weight"), ((2, 32, 64, 3, 9), "bwd_weight")]


@pytest.mark.parametrize("s5,kind", SCALE, ids=["%s-%s" % (_sid(s), k) for s, k in SCALE])
def test_bs3_power_of_two_scaling_is_exact(s5, kind):
    """x * 2^-40 with w * 2^12, dy * 2^30, no bias: every output is the unscaled one times the power of two, bit for bit (the split,
    the piece products and the fp32 sums commute with a power of two while nothing under- or overflows)."""
    L = cp.product_lib()
    x, w, dy = operands(full(s5))
    base = run3(L, kind, s5, x=x, w=w, dy=dy)
    tiny = 2.0 ** -126
    for name in (("out", "db") if kind == "bwd_weight" else ("out",)):
        v = base.out[name]
        assert bool(torch.isfinite(v).all()) and not bool(((v != 0) & (v.abs() < tiny)).any()), "an unscaled output is denormal"
    if kind == "fwd":
        r, f = run3(L, kind, s5, x=x * 2.0 ** -40, w=w * 2.0 ** 12), 2.0 ** -28
    elif kind == "bwd_data":
        r, f = run3(L, kind, s5, w=w * 2.0 ** 12, dy=dy * 2.0 ** 30), 2.0 ** 42
    else:
        r, f = run3(L, kind, s5, x=x * 2.0 ** -40, dy=dy * 2.0 ** 30), 2.0 ** -10
        assert bitwise_equal(r.out["db"], base.out["db"] * 2.0 ** 30)
    assert bitwise_equal(r.out["out"], base.out["out"] * f)


# --------------------------------------------------------------------------------------------- j: coherent errors
COHERENT = [("fwd", (3, 64, 64, 12, 8)), ("fwd", (1, 32, 64, 13, 13)), ("fwd", (1, 96, 64, 5, 33)), ("bwd_data", (2, 64, 32, 8, 8)),
            ("bwd_data", (2, 64, 64, 8, 12)), ("bwd_data", (1, 64, 96, 7, 27)), ("bwd_weight", (5, 64, 128, 6, 48)), ("bwd_weight", (1, 64, 32, 13, 13))]


@pytest.mark.parametrize("kind,s5", COHERENT, ids=["%s-%s" % (_sid(s), k) for k, s in COHERENT])
def test_bs3_error_is_that_of_an_fp32_chain(request, kind, s5):
    """All-positive operands at small, ragged shapes, one row per geometry and per weight-gradient kernel: (max, rms) of error / S
    must not exceed those of the f32 sibling (clhip_conv3x3_fwd / _bwd_data / _bwd_weight) on the same data — the claim behind
    `dtype: f32`."""
    L = cp.product_lib()
    shape = full(s5)
    x, w, dy = operands(shape, positive=True)
    want, cpu, Sabs = cp.ref_of(kind, reference(shape, positive=True))
    r = run3(L, kind, s5, x=x, w=w, dy=dy)
    f = run_f32(L, kind, s5, x, w, dy)
    bs, f32 = unit_errors(r.out["out"], want, Sabs), unit_errors(f.out["out"], want, Sabs)
    print("MEASURED|%s|error / S (max, rms) in units of 2^-24: bf16-split %.3f %.3f, f32 kernel %.3f %.3f|%.3f|%.3f"
          % (request.node.name, bs[0] / U, bs[1] / U, f32[0] / U, f32[1] / U, bs[0] / f32[0], bs[1] / f32[1]))
    assert bool(torch.isfinite(r.out["out"]).all())
    assert bs[0] <= f32[0] and bs[1] <= f32[1], "bf16-split %r against f32 %r" % (bs, f32)
