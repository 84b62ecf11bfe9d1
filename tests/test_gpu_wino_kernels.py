"""Kernel-level parity of the Winograd F(2x2, 3x3) kernels of csrc/wino.hip: clhip_conv3x3_wino_fwd / _bwd_data (wino_conv16_kernel,
wino_conv16g_kernel, wino_conv_kernel and the weight images they build), clhip_conv3x3_wino_bwd_weight (wino_wgrad_ps_kernel,
wino_wgrad_kernel and the slab reduction) and clhip_conv3x3_wino_bwd (wino_pair_kernel), called with raw pointers into one
kernel_parity.Arena (arg-max codes: a ByteArena beside it), each against the fp64 convolution of the same float32 inputs.

Dispatch.  wino_dispatch.py restates launch_wino, wino_wgrad_geo, clhip_internal_wino_pair and the workspace sizes; FWD_CASES,
WG_CASES and PAIR_CASES carry one hand-worked row per arm (test_wino_args_cpu.py checks the table without a GPU).  Every forward row
runs forward on the layer (C, K) = (Cin, Cout) and backward-data on the layer (C, K) = (Cout, Cin): the same kernel arm.
Observable: forward / backward-data write exactly wino_ws_bytes(Cin, Cout) bytes of weight images into the NaN workspace, the weight
gradient exactly splits * (9 K C + K) floats with splits from wgrad_geo (full and capped workspace), the merged grid both.

Accuracy rule, per element: |device - fp64| <= (R + 3) * 2^-24 * S_w[e] (+ 2^-24 |bias|), S_w the Winograd magnitude image of
kernel_parity.wino_magnitude / wino_wgrad_magnitude (every transform matrix and operand by absolute value).  R counts the roundings on
the path of one term, read from the kernels:
  forward / backward-data   weight transform t = G g, u = t G^T: each a three-term sum, 2 + 2 roundings (the factors 0.5 are exact);
      input transform B^T d B: row_tf, col_tf one subtraction each, 2; the product inside the MFMA 1; the channel sum: every
      kernel chains its MFMAs on one accumulator per frequency (v_mfma_f32_32x32x2 / 16x16x4, chunk after chunk, no tree and no LDS
      exchange), at most Cin additions; output transform u0 / u1 then y: 2 + 2; bias 1.  R = Cin + 12.
  weight gradient           A dY A^T 2, B^T d B 2, product 1, the sum over the N * ceil(H/2) * ceil(W/2) tiles of a block's share
      chained on one accumulator (zero tiles of the padded stages add exactly), in wino_wgrad_ps_kernel one more addition where the two
      tile halves meet through LDS, G^T M G 2 + 2, then `splits` slabs added in a fixed order.  R = N * tiles + splits + 9.
torch's float32 CPU convolution must meet the same bound (conv_parity.accuracy), which holds because S_w >= conv(|x|, |w|).  The rule
proves the absence of a wrong or missing term, not the quality of the rounding; test_wino_error_is_that_of_an_fp32_chain keeps
that in view.

Exact properties.  Out-channel 0 has zero weights and bias[0] = -0.0 (or no bias): every accumulator stays +0.0, the output transform
gives (+0) + (+0) and (+0) - (+0) = +0.0, and (+0.0) + (-0.0) = +0.0, so forward's channel 0 is +0.0 in every variant.  A masked
backward-data element is the literal 0.f: +0.0.  Fused pooling: `pool` is a run-time flag of ONE instantiation; both epilogues form
y00..y11 (+ bias, ReLU) by the same instructions before they part, so the pooled value is bit for bit the window maximum of the
unpooled output of the same call arguments.  Un-pooling: the staging writes (code == position ? dy : 0.f) into the LDS plane where the
dense form writes the dense dy's element, which torch_ref.unpool builds as the same value or +0.0; everything behind the LDS plane is
the same code, so the sums are the same bits (the un-pooling conv16<.,.,2> reads its weights from the LDS image where the dense one
reads the lane-ordered image: the same bits, test_wino_weight_images).  The weight gradient's scalar staging fills the same LDS
planes as the 16-byte staging: same bits.

Measured on one MI355X (device error / bound, float32-CPU error / bound, worst over the epilogue variants; run with -s):
  wino_conv_every_geometry (N,Cin,Cout,H,W)  arm              fwd             bwd_data (plain, mask, pooled dy on even maps)
  (3,16,32,8,8)                 conv16<1>        0.007 / 0.015   0.012 / 0.017
  (33,16,512,8,8)               conv16<2>        0.011 / 0.025   0.023 / 0.032      (pooled dy: the non-adirect instantiation)
  (79,16,512,8,8)               conv16g<4,4,4>   0.012 / 0.030   0.023 / 0.029
  (80,16,512,8,8)               conv16g<4,4,4>   0.012 / 0.023   0.026 / 0.036
  (3,24,96,4,16)                conv16g<8,2,4>   0.006 / 0.011   0.011 / 0.011
  (3,24,96,6,18)                conv16g<8,2,4>   0.006 / 0.010   0.012 / 0.016
  (3,24,96,10,32)               conv16g<8,2,4>   0.006 / 0.011   0.012 / 0.013
  (3,16,32,5,9)                 conv16g<8,2,1>   0.011 / 0.015   0.010 / 0.018
  (3,16,32,4,15)                conv16g<8,2,1>   0.008 / 0.013   0.009 / 0.018
  (3,16,32,13,16)               conv16g<8,2,1>   0.009 / 0.021   0.009 / 0.018
  (3,16,32,7,10)                conv16g<8,2,1>   0.008 / 0.019   0.009 / 0.016
  (5,16,32,4,8)                 conv32           0.008 / 0.016   0.014 / 0.013
  (5,16,32,6,10)                conv32           0.008 / 0.022   0.015 / 0.019
  (5,16,32,12,12)               conv32           0.008 / 0.021   0.016 / 0.027
  (5,16,32,8,14)                conv32           0.008 / 0.017   0.016 / 0.020
  (the rule is loose by design: Cin + 15 units of S_w, S_w = 4 - 17 x the direct magnitude; a dropped channel is far above it, see
  the mutation check)
  wino_fused_pool_is_exact, wino_unpooled_backward_data_is_exact, wino_unpooled_weight_gradient_is_exact: 0 windows with another code
  than the first maximum, values and gradients bit for bit, on every even row
  wino_weight_gradient_every_geometry: dw 0.000 - 0.011 of the bound on every row (float32 CPU 0.002 - 0.021); db at most 1.21 units of
  2^-24 sum|dy| (bounds 97 - 2053)
  wino_conv_operands_off_a_16_byte_boundary, wino_weight_gradient_operands_off_a_16_byte_boundary: bit for bit the aligned result with
  every operand 1 and 2 floats off, the scalar-staging weight gradient included
  wino_one_grid_backward: dx 0.002 - 0.007, dw 0.000 - 0.006 of the bound, db at most 0.46 units; dx / dw / db bit for bit the two
  launches' on the first two rows, dw / db on (33,512,64,8,8) — where dx was bit-identical too in this run, which the kernel's
  header does not promise and the test does not ask
  wino_weight_images: 0.38 - 0.53 of the 4-rounding bound, forward and backward-data images
  wino_error_is_that_of_an_fp32_chain, all-positive operands, error / S in units of 2^-24 (max, rms): Winograd | clhip_conv2d_*
  (3,16,32,8,8) fwd             10.6  1.84 | 10.9  2.83       ratio 0.97 0.65
  (3,24,96,6,18) fwd            13.2  1.84 | 15.7  3.27       ratio 0.84 0.56
  (5,16,32,6,10) fwd            11.6  1.86 | 11.9  2.67       ratio 0.98 0.70
  (3,96,24,6,18) bwd_data       13.4  1.84 | 13.0  3.29       ratio 1.03 0.56
  (2,64,64,8,8) bwd_weight      4.93  1.11 | 12.7  2.54       ratio 0.39 0.44
  (4,64,64,16,16) bwd_weight    17.0  4.62 | 8.41  2.02       ratio 2.02 2.29    (wino_wgrad_kernel on one slab: a chain of 1024 tiles)
  Run time on the MI355X: 116 tests in 8.5 s; 0.52 s for the largest (80,16,512,8,8) backward-data case, 0.23 s for the first test
  (library load), at most 0.32 s for any other.

Found and fixed with these tests: (1) clhip_conv3x3_wino_fwd / _bwd_data on an odd map with arg-max codes answered CLHIP_ENOTSUP
only after the weight transform had been launched (wino_refused_calls_write_nothing on the parent library: rc -3, workspace
written); the refusal now stands ahead of the launch.  (2) clhip_internal_wino_wgrad_ok took C = 0 or K = 0, and the slab counts then
divided by zero (test_wino_args_cpu.py on the parent library: the process dies of SIGFPE); it asks for C, K > 0 now.

Mutation check, run once against scratch copies of the sources (one run of this file per mutant with CLHIP_LIB on the mutant
library; only load predicates, loop trip counts downwards and comparisons change, no store index does, so each stays in bounds; not
part of the repository):
  (a) conv16g staging: `h < H - 1` (the map's last row reads 0)      28 fail: every conv16g row of conv_every_geometry x18, the conv16g rows
                                                                      of conv_operands_off... x4, one_grid_backward on the two rows that
                                                                      hold the conv16g body x4, error_is_that_of_an_fp32_chain x2
  (b) conv16g: n_chunks = (Cin / 16) * 4 (one 8-channel chunk short   10 fail: exactly the Cin = 24 rows — conv_every_geometry x6,
      at Cin = 24, right at 16 and 64)                                conv_operands_off... x2, error_is_that_of_an_fp32_chain x2
  (c) `m0.x >= 0.f` in the even-map mask of conv16g / conv16 / conv32  8 / 4 / 5 fail: the backward-data cases of conv_every_geometry on that
      (three mutants)                                                 kernel's rows, conv_operands_off... on its row, one_grid_backward plain
  (d) un-pooling `code <= position` for `==` in conv16g / conv16 /    11 / 5 / 8 fail: backward-data of conv_every_geometry and
      conv32 (three mutants)                                          unpooled_backward_data_is_exact on that kernel's even rows, one_grid_backward pooled
  (e) ... in wino_wgrad_ps_kernel (`cde <= 1`) / wino_wgrad_kernel    11 / 8 fail: the pooled rows of weight_gradient_every_geometry and
      (two mutants)                                                   unpooled_weight_gradient_is_exact on that kernel, one_grid_backward pooled x3 (ps)
  (f) clhip_conv3x3_wino_bwd_weight reduces splits + 1 slabs          run on the rows whose workspace holds more slabs than the launch takes
                                                                      (-k "every_geometry and full", so that the extra slab is inside the
                                                                      workspace): 14 of 14 fail (the sentinel slab makes dw non-finite)
No mutant survived.
"""
import functools

import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

import conv_dispatch as cd
import conv_parity as cp
import torch_ref
import wino_dispatch as wd
from conv_parity import BYTE_OUT, OUT_BITS, U, WS_BITS, WS_SLACK, accuracy, check_ws, run_call, unit_errors
from kernel_parity import CPU_FACTOR, all_bits, bitwise_equal, wino_magnitude, wino_wgrad_magnitude

pytestmark = pytest.mark.gpu

ENOTSUP = -3
FWD_GPU = [row for row in wd.FWD_CASES if row[0][0] != 78]         # N = 78 differs from N = 33 by the block count only: table row only


def full(s5):
    """Layer (N, C, K, H, W) -> the (N, C, H, W, K, R, S, stride, pad) of conv_parity."""
    N, Cc, K, H, W = s5
    return (N, Cc, H, W, K, 3, 3, 1, 1)


@functools.lru_cache(maxsize=None)
def seed_of(shape):
    """The first seed whose draws hold no exact zero (conv_parity.operands asserts that; seed 0 draws one for (5,32,16,6,10))."""
    for seed in range(8):
        try:
            cp.operands(shape, seed)
            return seed
        except AssertionError:
            pass
    raise AssertionError("no seed without a zero for %r" % (shape,))


def operands(shape, positive=False):
    return cp.operands(shape, seed_of(shape), positive)


def reference(shape, positive=False):
    return cp.reference(shape, seed_of(shape), positive)


def layer_of(kind, row):
    """The layer whose forward (kind fwd) / backward-data puts the kernel on the (Cin, Cout) of a FWD_CASES row."""
    N, Cin, Cout, H, W = row
    return (N, Cin, Cout, H, W) if kind == "fwd" else (N, Cout, Cin, H, W)


def _sid(s5):
    return "x".join(str(v) for v in s5)


def codes_for(N, K, OH, OW, seed=0):
    """Arg-max codes 0..4 for every window: random, with whole planes of one code (runs of equal codes, 4 = dead among them) in the
    first image's first channels and every code at every window position somewhere."""
    gen = torch.Generator().manual_seed(4242 + seed + N * K + OH * OW)
    code = torch.randint(0, 5, (N, K, OH, OW), generator=gen, dtype=torch.uint8)
    for c in range(min(5, K)):
        code[0, c] = c
    code[N - 1, K - 1] = (torch.arange(OH * OW) % 5).to(torch.uint8).view(OH, OW)                    # cycles through the codes
    return code


def pooled_dy(s5, seed=0):
    """(pooled gradient, codes, the dense dy torch_ref.unpool builds from them)."""
    N, Cc, K, H, W = s5
    gen = torch.Generator().manual_seed(99 + seed + N * K * H * W)
    dyp = torch.randn((N, K, H // 2, W // 2), generator=gen)
    assert bool((dyp != 0).all())
    code = codes_for(N, K, H // 2, W // 2, seed)
    return dyp, code, torch_ref.unpool(dyp, code)


def rot_t(w):
    """The weights as backward-data's kernel sees them: g[c][k] = the 180-degree-rotated w[k][c]."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv_ref(kind, s5, pooled=False, positive=False):
    """(fp64 result, float32 CPU result, Winograd magnitude, direct magnitude) of forward / backward-data on the shared operands."""
    shape = full(s5)
    x, w, dy = operands(shape, positive=positive)
    if kind == "fwd":
        ref = reference(shape, positive=positive)
        return ref.y64, ref.y32, wino_magnitude(x, w), ref.s_y
    if pooled:
        dy = pooled_dy(s5)[2]
        want, cpu = conv2d_input(x.shape, w.double(), dy.double(), 1, 1), conv2d_input(x.shape, w, dy, 1, 1)
        return want, cpu, wino_magnitude(dy, rot_t(w)), None
    ref = reference(shape, positive=positive)
    return ref.dx64, ref.dx32, wino_magnitude(dy, rot_t(w)), ref.s_dx


@functools.lru_cache(maxsize=None)
def wgrad_ref(s5, pooled=False, positive=False):
    """(dw fp64, dw float32 CPU, S_wg, direct magnitude, db fp64, sum |dy|) of the weight gradient on the shared operands."""
    shape = full(s5)
    x, w, dy = operands(shape, positive=positive)
    if pooled:
        dy = pooled_dy(s5)[2]
        dw64, dw32 = conv2d_weight(x.double(), w.shape, dy.double(), 1, 1), conv2d_weight(x, w.shape, dy, 1, 1)
        return dw64, dw32, wino_wgrad_magnitude(x, dy), None, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
    ref = reference(shape, positive=positive)
    return ref.dw64, ref.dw32, wino_wgrad_magnitude(x, dy), ref.s_dw, ref.db64, ref.s_db


# --------------------------------------------------------------------------------------------- raw-pointer calls
def run_fwd(L, s5, x, w, bias=None, relu=0, pool=False, ws_bytes=None, mis=None, mis_by=1):
    N, Cc, K, H, W = s5
    need = wd.wino_ws_bytes(Cc, K) if ws_bytes is None else ws_bytes
    n_out = N * K * (H // 2) * (W // 2) if pool else N * K * H * W

    def call(p, ws, nbytes, stream):
        return L.clhip_conv3x3_wino_fwd(p["x"], p["w"], p["b"], p["out"], p["idx"], N, Cc, K, H, W, int(relu), ws, nbytes, stream)
    return run_call(call, [("x", x), ("w", w), ("b", bias)], [("out", n_out)], ws_floats=need // 4 + WS_SLACK, ws_bytes=need, mis=mis,
                    mis_by=mis_by, bouts=[("idx", n_out if pool else None)])


def run_bwd_data(L, s5, dy, w, src=None, code=None, ws_bytes=None, mis=None, mis_by=1):
    """dy: the dense gradient, or with `code` the pooled one."""
    N, Cc, K, H, W = s5
    need = wd.wino_ws_bytes(K, Cc) if ws_bytes is None else ws_bytes

    def call(p, ws, nbytes, stream):
        return L.clhip_conv3x3_wino_bwd_data(p["dy"], p["idx"], p["w"], p["src"], p["out"], N, Cc, K, H, W, ws, nbytes, stream)
    return run_call(call, [("dy", dy), ("w", w), ("src", src)], [("out", N * Cc * H * W)], ws_floats=need // 4 + WS_SLACK, ws_bytes=need,
                    mis=mis, mis_by=mis_by, bins=[("idx", code)])


def run_wgrad(L, s5, x, dy, code=None, want_db=True, ws_bytes=None, mis=None, mis_by=1):
    N, Cc, K, H, W = s5
    need = wd.wgrad_ws_bytes(*s5) if ws_bytes is None else ws_bytes

    def call(p, ws, nbytes, stream):
        return L.clhip_conv3x3_wino_bwd_weight(p["x"], p["dy"], p["idx"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    return run_call(call, [("x", x), ("dy", dy)], [("out", K * Cc * 9), ("db", K if want_db else None), ("nodb", None if want_db else K)],
                    ws_floats=need // 4 + WS_SLACK, ws_bytes=need, mis=mis, mis_by=mis_by, bins=[("idx", code)])


def run_pair(L, s5, x, dy, w, src=None, code=None):
    N, Cc, K, H, W = s5
    need = wd.wino_bwd_ws_bytes(*s5)

    def call(p, ws, nbytes, stream):
        return L.clhip_conv3x3_wino_bwd(p["x"], p["dy"], p["idx"], p["w"], p["src"], p["dx"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    return run_call(call, [("x", x), ("dy", dy), ("w", w), ("src", src)], [("dx", N * Cc * H * W), ("out", K * Cc * 9), ("db", K)],
                    ws_floats=need // 4 + WS_SLACK, ws_bytes=need, bins=[("idx", code)])


def run_f32(L, kind, s5, x, w, dy):
    """The f32 sibling of the same operator on the same data: clhip_conv2d_fwd / _bwd_data / _bwd_weight."""
    shape = full(s5)
    N, Cc, K, H, W = s5
    if kind == "fwd":
        ins, outs = [("x", x), ("w", w)], [("out", N * K * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_fwd(p["x"], p["w"], None, p["out"], *shape, 0, stream)
    elif kind == "bwd_data":
        ins, outs = [("dy", dy), ("w", w)], [("out", N * Cc * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_data(p["dy"], p["w"], None, p["out"], *shape, stream)
    else:
        ins, outs = [("x", x), ("dy", dy)], [("out", K * Cc * 9)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_weight(p["x"], p["dy"], p["out"], None, *shape, ws, nbytes, stream)
    r = run_call(call, ins, outs, ws_floats=cd.bwd_weight_ws_bytes(shape) // 4)
    assert r.rc == 0 and r.clean
    return r


def ok_call(r, what, img_floats):
    assert r.rc == 0 and r.clean, "%s: rc %d, gaps, guards or inputs changed: %s" % (what, r.rc, not r.clean)
    check_ws(r.ws, img_floats, what)


# --------------------------------------------------------------------------------------------- a. forward / backward-data
CONV = [(row, k) for row, _ in FWD_GPU for k in ("fwd", "bwd_data")]


def check_conv(case, L, kind, row, only=None, mis=None, mis_by=1):
    """Every epilogue variant of one FWD_CASES row: rc, clean arena, exactly the weight images written, every output element
    written and within the rule, exact epilogue semantics.  Returns the outputs by variant name."""
    N, Cin, Cout, H, W = row
    s5 = layer_of(kind, row)
    Cc, K = s5[1], s5[2]
    x, w, dy = operands(full(s5))
    bias, src = cp.epilogue_inputs(full(s5))
    img = wd.wino_ws_bytes(Cin, Cout) // 4
    R = Cin + 12
    outs = {}
    if kind == "fwd":
        want, cpu, Sw, _ = conv_ref("fwd", s5)
        for name, kw, acc in (("bias-relu", dict(bias=bias, relu=1), dict(bias=bias, relu=True)), ("bias", dict(bias=bias), dict(bias=bias)),
                              ("plain", {}, {}), ("relu", dict(relu=1), dict(relu=True))):
            if only is not None and name != only:
                continue
            r = run_fwd(L, s5, x, w, mis=mis, mis_by=mis_by, **kw)
            ok_call(r, name, img)
            accuracy(case, name, r.out["out"], want, cpu, Sw, R, 0, **acc)
            outs[name] = r.out["out"]
            # zero weights, bias -0.0 or none: +0.0 (see the header)
            assert all_bits(outs[name].view(N, K, H, W)[:, 0], 0), "%s: out-channel 0 must be exactly +0.0" % name
        if only is None:
            assert torch.equal(outs["bias-relu"], outs["bias"].clamp(min=0)) and torch.equal(outs["relu"], outs["plain"].clamp(min=0)), \
                "relu is not max(v, 0) of the same v"
        return outs
    want, cpu, Sw, _ = conv_ref("bwd_data", s5)
    for name, kw, acc in (("relu_src", dict(src=src), dict(mask_src=src)), ("plain", {}, {})):
        if only is not None and name != only:
            continue
        r = run_bwd_data(L, s5, dy, w, mis=mis, mis_by=mis_by, **kw)
        ok_call(r, name, img)
        accuracy(case, name, r.out["out"], want, cpu, Sw, R, 0, **acc)
        outs[name] = r.out["out"]
    if only is None:
        on = src.reshape(-1) > 0
        assert bitwise_equal(outs["relu_src"][on], outs["plain"][on]), "relu_src > 0 must pass the value through unchanged"
        assert all_bits(outs["relu_src"][~on], 0), "relu_src of 0.0, -0.0, a negative denormal, NaN or a negative must give exactly +0.0"
    if (H | W) & 1 or only is not None:
        return outs
    dyp, code, dense = pooled_dy(s5)                       # pooled dy + codes, plain and behind a mask
    want, cpu, Sw, _ = conv_ref("bwd_data", s5, pooled=True)
    for name, kw, acc in (("pooled", {}, {}), ("pooled-relu_src", dict(src=src), dict(mask_src=src))):
        r = run_bwd_data(L, s5, dyp, w, code=code, **kw)
        ok_call(r, name, img)
        accuracy(case, name, r.out["out"], want, cpu, Sw, R, 0, **acc)
        outs[name] = r.out["out"]
    return outs


@pytest.mark.parametrize("row,kind", CONV, ids=["%s-%s" % (_sid(r), k) for r, k in CONV])
def test_wino_conv_every_geometry(request, row, kind):
    """Every arm of launch_wino, forward and backward-data (with pooled dy + codes on even maps), every epilogue variant."""
    L = cp.product_lib()
    plan = dict(wd.FWD_CASES)[row]
    assert wd.fwd_plan(*row) == plan and L.clhip_conv3x3_wino_ws(row[1], row[2]) >= wd.wino_ws_bytes(row[1], row[2])
    check_conv(request.node.name, L, kind, row)


# --------------------------------------------------------------------------------------------- b. fused pooling, exact
POOL_ROWS = [row for row, _ in FWD_GPU if not (row[3] | row[4]) & 1 and row[0] != 80]


@pytest.mark.parametrize("row", POOL_ROWS, ids=[_sid(r) for r in POOL_ROWS])
def test_wino_fused_pool_is_exact(row):
    """The pooled forward against the device's own unpooled output of the same arguments: value = the window maximum bit for bit,
    code = the first maximum in row-major order, or 4 under ReLU where the maximum is not positive (idx == 4 iff y == 0).  Planted
    ties: out-channel 0 (all four +0.0: code 0 plain, 4 under ReLU), out-channel 1 with zero weights and bias 0.25 (code 0 in both)."""
    L = cp.product_lib()
    N, Cc, K, H, W = row
    x, w, _ = operands(full(row))
    bias, _ = cp.epilogue_inputs(full(row))
    w, bias = w.clone(), bias.clone()
    w[1] = 0.0
    bias[1] = 0.25
    img = wd.wino_ws_bytes(Cc, K) // 4
    for relu in (0, 1):
        dense = run_fwd(L, row, x, w, bias=bias, relu=relu)
        ok_call(dense, "unpooled", img)
        r = run_fwd(L, row, x, w, bias=bias, relu=relu, pool=True)
        ok_call(r, "pooled", img)
        y, idx = r.out["out"].view(N, K, H // 2, W // 2), r.out["idx"].view(N, K, H // 2, W // 2)
        assert not bool((idx == BYTE_OUT).any()) and not bool((y.view(torch.int32) == OUT_BITS).any()), "a window was never written"
        win = dense.out["out"].view(N, K, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, K, H // 2, W // 2, 4)
        m, a = win[..., 0].clone(), torch.zeros(idx.shape, dtype=torch.uint8)
        for i in (1, 2, 3):
            gt = win[..., i] > m
            m, a = torch.where(gt, win[..., i], m), torch.where(gt, torch.full_like(a, i), a)
        if relu:
            a = torch.where(m > 0, a, torch.full_like(a, 4))
        wrong = int((idx != a).sum())
        print("MEASURED|%s|relu %d: windows with another code than the first maximum|%d|0" % (_sid(row), relu, wrong))
        assert bitwise_equal(y, m), "the pooled value is not the maximum of the unpooled output's window"
        assert wrong == 0, "%d codes are not the first maximum in row-major order" % wrong
        assert int(idx.max()) <= (4 if relu else 3)
        if relu:
            assert torch.equal(idx == 4, y == 0)
        assert bool((idx[:, 0] == (4 if relu else 0)).all()) and all_bits(y[:, 0], 0), "out-channel 0: four equal +0.0"
        assert bool((idx[:, 1] == 0).all()) and bool((y[:, 1] == 0.25).all()), "out-channel 1: four equal positive values"


# --------------------------------------------------------------------------------------------- c. un-pooling, exact
@pytest.mark.parametrize("row", POOL_ROWS, ids=[_sid(r) for r in POOL_ROWS])
def test_wino_unpooled_backward_data_is_exact(row):
    """Backward-data from (pooled dy, codes) = backward-data from the dense dy torch_ref.unpool builds, bit for bit."""
    L = cp.product_lib()
    s5 = layer_of("bwd_data", row)
    _, w, _ = operands(full(s5))
    dyp, code, dense = pooled_dy(s5)
    assert set(code.reshape(-1).tolist()) == {0, 1, 2, 3, 4}
    a = run_bwd_data(L, s5, dyp, w, code=code)
    b = run_bwd_data(L, s5, dense, w)
    assert a.rc == 0 and a.clean and b.rc == 0 and b.clean
    assert bitwise_equal(a.out["out"], b.out["out"]), "dx from pooled dy + codes differs from dx of the dense gradient"


# --------------------------------------------------------------------------------------------- d. weight gradient
def check_wgrad(case, L, wcase, mis=None, mis_by=1, want_db=True):
    s5, pooled, slabs, aligned, geo = wcase
    N, Cc, K, H, W = s5
    x, w, dy = operands(full(s5))
    code = None
    if pooled:
        dy, code, _ = pooled_dy(s5)
    dw64, dw32, Swg, _, db64, s_db = wgrad_ref(s5, pooled)
    ws_bytes = wd.wg_ws_bytes(wcase)
    if mis is None and not aligned:
        mis = "x"
    g = wd.wgrad_geo(*s5, ws_bytes, mis not in ("x", "dy"), pooled)
    touched = g.splits * wd.slab_floats(Cc, K)
    r = run_wgrad(L, s5, x, dy, code=code, want_db=want_db, ws_bytes=ws_bytes, mis=mis, mis_by=mis_by)
    ok_call(r, case, touched)
    tiles = ((H + 1) // 2) * ((W + 1) // 2)
    accuracy(case, "dw", r.out["out"], dw64, dw32, Swg, N * tiles + 9, g.splits)
    if want_db:
        e = float(((r.out["db"].double() - db64).abs() / (U * s_db)).max())
        print("MEASURED|%s|db error in units of 2^-24 sum abs(dy), bound %d|%.3f|-" % (case, N * H * W + g.splits + 3, e))
        assert bool(torch.isfinite(r.out["db"]).all()) and e <= N * H * W + g.splits + 3, "db: %.3f units" % e
    else:
        assert all_bits(r.out["nodb"], OUT_BITS), "db = NULL: the db-sized slot must keep its sentinel"
    return r


WG_IDS = ["%s-%s-%s-%s" % (_sid(c[0]), "pooled" if c[1] else "plain", "full" if c[2] is None else "%dslab" % c[2], "al" if c[3] else "mis") for c in wd.WG_CASES]


@pytest.mark.parametrize("wcase", wd.WG_CASES, ids=WG_IDS)
def test_wino_weight_gradient_every_geometry(request, wcase):
    """Every arm of wino_wgrad_geo (both kernels, wide / narrow, 16-byte / scalar staging, plain / un-pooling), on the workspace the
    row hands over: exactly splits slabs written, dw and db by the rules, db = NULL, a second call the same bits."""
    L = cp.product_lib()
    case = request.node.name
    s5, pooled, slabs, aligned, geo = wcase
    assert wd.wgrad_geo(*s5, wd.wg_ws_bytes(wcase), aligned, pooled) == geo
    assert L.clhip_conv3x3_wino_bwd_weight_ws(*s5) >= wd.wgrad_ws_bytes(*s5) > 0
    r = check_wgrad(case, L, wcase)
    r2 = check_wgrad(case + "[again]", L, wcase)
    assert bitwise_equal(r.out["out"], r2.out["out"]) and bitwise_equal(r.out["db"], r2.out["db"]), "two calls differ"
    r3 = check_wgrad(case + "[db=NULL]", L, wcase, want_db=False)
    assert bitwise_equal(r.out["out"], r3.out["out"]), "dw must not depend on db being asked for"


UNPOOL_WG = [c for c in wd.WG_CASES if c[1]]


@pytest.mark.parametrize("wcase", UNPOOL_WG, ids=[i for i, c in zip(WG_IDS, wd.WG_CASES) if c[1]])
def test_wino_unpooled_weight_gradient_is_exact(wcase):
    """dw, db from (pooled dy, codes) = dw, db from the dense dy torch_ref.unpool builds, bit for bit, on the same workspace."""
    L = cp.product_lib()
    s5, pooled, slabs, aligned, geo = wcase
    x, _, _ = operands(full(s5))
    dyp, code, dense = pooled_dy(s5)
    a = run_wgrad(L, s5, x, dyp, code=code, ws_bytes=wd.wg_ws_bytes(wcase))
    b = run_wgrad(L, s5, x, dense, ws_bytes=wd.wg_ws_bytes(wcase))
    assert a.rc == 0 and a.clean and b.rc == 0 and b.clean
    assert bitwise_equal(a.out["out"], b.out["out"]) and bitwise_equal(a.out["db"], b.out["db"])


# --------------------------------------------------------------------------------------------- e. off a 16-byte boundary
MIS_ROWS = [((3, 16, 32, 8, 8), "conv16"), ((3, 24, 96, 6, 18), "conv16g"), ((3, 16, 32, 5, 9), "conv16g"), ((5, 16, 32, 6, 10), "conv32")]
MIS = [(row, k) for row, _ in MIS_ROWS for k in ("fwd", "bwd_data")]


@pytest.mark.parametrize("row,kind", MIS, ids=["%s-%s" % (_sid(r), k) for r, k in MIS])
def test_wino_conv_operands_off_a_16_byte_boundary(request, row, kind):
    """x, w, bias, y (forward) / dy, w, mask, dx (backward-data) in turn one and two floats past a 16-byte boundary, one row per
    kernel family (and the row-packed odd geometry): clean, within the rule, and — no path of these kernels depends on an
    operand's alignment — the aligned result's bits."""
    L = cp.product_lib()
    assert wd.fwd_plan(*row).kernel == dict(MIS_ROWS)[row]
    variant = "bias-relu" if kind == "fwd" else "relu_src"
    base = check_conv(request.node.name, L, kind, row, only=variant)[variant]
    for name in (("x", "w", "b", "out") if kind == "fwd" else ("dy", "w", "src", "out")):
        for by in (1, 2):
            got = check_conv("%s[%s+%d]" % (request.node.name, name, by), L, kind, row, only=variant, mis=name, mis_by=by)[variant]
            assert bitwise_equal(got, base), "%s %d floats off: the result changed" % (name, by)


MIS_WG = [c for c in wd.WG_CASES if c[3] and not c[1] and (c[0], c[2]) in (((2, 64, 64, 8, 8), None), ((2, 64, 64, 4, 16), None),
                                                                         ((4, 64, 64, 16, 16), 1), ((16, 64, 64, 8, 8), 1))]


@pytest.mark.parametrize("wcase", MIS_WG, ids=["%s-%s" % (_sid(c[0]), "ps" if c[4].ps else "wg") for c in MIS_WG])
def test_wino_weight_gradient_operands_off_a_16_byte_boundary(request, wcase):
    """x, dy, dw, db in turn one and two floats off, both kernels, wide and narrow.  A misaligned x or dy selects the scalar-staging
    instantiation of the same kernel: it fills the same LDS planes with the same values, the sums behind them are the same code, so
    the result is the 16-byte-staged one bit for bit."""
    L = cp.product_lib()
    assert len(MIS_WG) == 4 and wcase[4].vec
    base = check_wgrad(request.node.name, L, wcase)
    for name in ("x", "dy", "out", "db"):
        for by in (1, 2):
            r = check_wgrad("%s[%s+%d]" % (request.node.name, name, by), L, wcase, mis=name, mis_by=by)
            assert bitwise_equal(r.out["out"], base.out["out"]) and bitwise_equal(r.out["db"], base.out["db"]), \
                "%s %d floats off: the result changed" % (name, by)


# --------------------------------------------------------------------------------------------- f. merged backward grid
PAIR = [(s, pooled) for s, _ in wd.PAIR_CASES for pooled in (False, True)]


@pytest.mark.parametrize("s5,pooled", PAIR, ids=["%s-%s" % (_sid(s), "pooled" if p else "plain") for s, p in PAIR])
def test_wino_one_grid_backward(request, s5, pooled):
    """clhip_conv3x3_wino_bwd: exactly the backward-data weight images and the slabs written, dx / dw / db by the rules and bit for bit
    those of the two launches — except dx on the PAIR(0,4,4) row, where launch_wino runs conv16<1,.,2> and the grid the conv16g body
    (the same sums in another order): the rule alone there."""
    L = cp.product_lib()
    case = request.node.name
    N, Cc, K, H, W = s5
    plan = dict(wd.PAIR_CASES)[s5]
    assert wd.pair_plan(*s5, pooled) == plan
    x, w, dy = operands(full(s5))
    _, src = cp.epilogue_inputs(full(s5))
    code = None
    if pooled:
        dy, code, _ = pooled_dy(s5)
        src = None                                         # behind a fused pool the plan passes no ReLU source
    r = run_pair(L, s5, x, dy, w, src=src, code=code)
    assert wd.bwd_u_bytes(Cc, K) == wd.wino_ws_bytes(K, Cc)          # no padding between the images and the slabs at these shapes
    ok_call(r, case, wd.wino_ws_bytes(K, Cc) // 4 + plan.splits * wd.slab_floats(Cc, K))
    want, cpu, Sw, _ = conv_ref("bwd_data", s5, pooled)
    accuracy(case, "dx", r.out["dx"], want, cpu, Sw, K + 12, 0, mask_src=src)
    dw64, dw32, Swg, _, db64, s_db = wgrad_ref(s5, pooled)
    accuracy(case, "dw", r.out["out"], dw64, dw32, Swg, N * (H // 2) * (W // 2) + 9, plan.splits)
    e = float(((r.out["db"].double() - db64).abs() / (U * s_db)).max())
    print("MEASURED|%s|db error in units of 2^-24 sum abs(dy), bound %d|%.3f|-" % (case, N * H * W + plan.splits + 3, e))
    assert bool(torch.isfinite(r.out["db"]).all()) and e <= N * H * W + plan.splits + 3
    d = run_bwd_data(L, s5, dy, w, src=src, code=code)
    g = run_wgrad(L, s5, x, dy, code=code)
    assert d.rc == 0 and d.clean and g.rc == 0 and g.clean
    assert wd.wgrad_geo(*s5, wd.wgrad_ws_bytes(*s5), True, pooled).splits == plan.splits
    assert bitwise_equal(r.out["out"], g.out["out"]) and bitwise_equal(r.out["db"], g.out["db"]), "dw / db differ from the launch of their own"
    if (plan.dk, plan.tc) == (0, 4):
        assert wd.fwd_plan(N, K, Cc, H, W).kernel == "conv16"
        print("MEASURED|%s|dx bit for bit the two launches' (not required here)|%d|-" % (case, bitwise_equal(r.out["dx"], d.out["out"])))
    else:
        assert bitwise_equal(r.out["dx"], d.out["out"]), "dx differs from the launch of its own"


# --------------------------------------------------------------------------------------------- g. weight images
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("Cin,Cout", [(24, 96), (16, 32), (72, 160)])
def test_wino_weight_images(Cin, Cout, mode):
    """Both images of U = G g G^T at ragged out-channel counts, as forward (mode 0) and backward-data (mode 1: the rotated,
    transposed weights) build them: the same bits in the LDS image and the lane-ordered image, zero in the out-channels past Cout
    and in the 4 pad floats, values within 4 roundings (2 + 2 of the two three-term sums) of the fp64 G g G^T."""
    import numpy as np
    L = cp.product_lib()
    s5 = (1, Cin, Cout, 8, 8) if mode == 0 else (1, Cout, Cin, 8, 8)
    x, w, dy = operands(full(s5))
    r = run_fwd(L, s5, x, w) if mode == 0 else run_bwd_data(L, s5, dy, w)
    g = (w if mode == 0 else rot_t(w)).double().numpy()                         # [Cout][Cin][3][3] as the kernel sees it
    kts, nch = (Cout + 63) // 64, Cin // 8
    n_lds, n_dir = kts * nch * 8 * 64 * 20, kts * nch * 2 * 4096
    ok_call(r, "images", n_lds + n_dir)
    assert 4 * (n_lds + n_dir) == wd.wino_ws_bytes(Cin, Cout)
    Uimg = r.ws.numpy()
    lds = Uimg[:n_lds].reshape(kts, nch, 8, 64, 20)
    assert np.all(lds[..., 16:].view(np.uint32) == 0), "the 4 pad floats"
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
    want, mag = np.zeros((kts * 64, Cin, 16)), np.zeros((kts * 64, Cin, 16))
    want[:Cout] = np.einsum("ar,kcrs,bs->kcab", G, g, G).reshape(Cout, Cin, 16)
    mag[:Cout] = np.einsum("ar,kcrs,bs->kcab", np.abs(G), np.abs(g), np.abs(G)).reshape(Cout, Cin, 16)
    got = lds[..., :16].transpose(0, 3, 1, 2, 4).reshape(kts * 64, Cin, 16)    # [k][c][f]
    assert np.all(got[Cout:].view(np.uint32) == 0), "out-channels past Cout"
    worst = float((np.abs(got - want)[:Cout] / (4 * U * mag[:Cout]).clip(min=1e-300)).max())
    print("MEASURED|%d->%d mode %d|U against fp64 G g G^T in units of 4 * 2^-24 abs(G) abs(g) abs(G^T)|%.3f|-" % (Cin, Cout, mode, worst))
    assert worst <= 1.0
    direct = Uimg[n_lds:n_lds + n_dir].reshape(kts, 2 * nch, 2, 2, 4, 4, 16, 4)  # kt, chunk4, wk, r, fq, q, ti, j
    e = lds[..., :16].reshape(kts, nch, 2, 4, 2, 2, 16, 4, 4)                   # kt, chunk8, half, q, wk, r, ti, fq, j
    e = e.transpose(0, 1, 2, 4, 5, 7, 3, 6, 8).reshape(kts, 2 * nch, 2, 2, 4, 4, 16, 4)
    assert np.array_equal(direct.view(np.uint32), np.ascontiguousarray(e).view(np.uint32)), "the two images differ"


# --------------------------------------------------------------------------------------------- h. refused calls write nothing
def test_wino_refused_calls_write_nothing():
    """Arg-max codes on an odd map: CLHIP_ENOTSUP from every entry point, outputs and workspace on their sentinels (forward and
    backward-data refuse ahead of the weight transform)."""
    L = cp.product_lib()
    s5 = (3, 64, 64, 5, 9)
    N, Cc, K, H, W = s5
    x, w, dy = operands(full(s5))
    code = torch.zeros((N * K * 2 * 4,), dtype=torch.uint8)
    dyp = torch.ones((N * K * 2 * 4,))

    def fwd(p, ws, nbytes, stream):
        return L.clhip_conv3x3_wino_fwd(p["x"], p["w"], None, p["out"], p["idx"], N, Cc, K, H, W, 1, ws, nbytes, stream)
    big = wd.wino_bwd_ws_bytes(*s5)
    r = run_call(fwd, [("x", x), ("w", w)], [("out", N * K * H * W)], ws_floats=big // 4, bouts=[("idx", N * K * 8)])
    assert r.rc == ENOTSUP and r.clean and all_bits(r.out["out"], OUT_BITS) and all_bits(r.ws, WS_BITS) and bool((r.out["idx"] == BYTE_OUT).all()), \
        "forward: rc %d, workspace written: %s" % (r.rc, not all_bits(r.ws, WS_BITS))
    r = run_bwd_data(L, s5, dyp, w, code=code, ws_bytes=big)
    assert r.rc == ENOTSUP and r.clean and all_bits(r.out["out"], OUT_BITS) and all_bits(r.ws, WS_BITS), \
        "backward-data: rc %d, workspace written: %s" % (r.rc, not all_bits(r.ws, WS_BITS))
    r = run_wgrad(L, s5, x, dyp, code=code, ws_bytes=big)
    assert r.rc == ENOTSUP and r.clean and all_bits(r.out["out"], OUT_BITS) and all_bits(r.out["db"], OUT_BITS) and all_bits(r.ws, WS_BITS)
    for c in (code, None):
        r = run_pair(L, s5, x, dyp if c is not None else dy, w, code=c)
        assert r.rc == ENOTSUP and r.clean and all(all_bits(r.out[k], OUT_BITS) for k in ("dx", "out", "db")) and all_bits(r.ws, WS_BITS)


# --------------------------------------------------------------------------------------------- quality of the rounding
COHERENT = [("fwd", (3, 16, 32, 8, 8)), ("fwd", (3, 24, 96, 6, 18)), ("fwd", (5, 16, 32, 6, 10)), ("bwd_data", (3, 96, 24, 6, 18)),
            ("bwd_weight", (2, 64, 64, 8, 8)), ("bwd_weight", (4, 64, 64, 16, 16))]


@pytest.mark.parametrize("kind,s5", COHERENT, ids=["%s-%s" % (_sid(s), k) for k, s in COHERENT])
def test_wino_error_is_that_of_an_fp32_chain(request, kind, s5):
    """All-positive operands: rounding errors add up instead of cancelling.  In units of 2^-24 * S[e], S the DIRECT magnitude
    conv(|x|, |w|) (max and rms), the Winograd kernel's error must not exceed CPU_FACTOR = 4 x that of clhip_conv2d_* on the same
    data; one row per kernel family (conv16, conv16g, conv32; wino_wgrad_ps_kernel, wino_wgrad_kernel on one slab)."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    x, w, dy = operands(full(s5), positive=True)
    if kind == "fwd":
        want, _, _, S = conv_ref("fwd", s5, positive=True)
        r = run_fwd(L, s5, x, w)
    elif kind == "bwd_data":
        want, _, _, S = conv_ref("bwd_data", s5, positive=True)
        r = run_bwd_data(L, s5, dy, w)
    else:
        want, _, _, S = wgrad_ref(s5, positive=True)[:4]
        r = run_wgrad(L, s5, x, dy, ws_bytes=wd.slab_floats(Cc, K) * 4 if H == 16 else None)
    assert r.rc == 0 and r.clean and bool(torch.isfinite(r.out["out"]).all())
    f = run_f32(L, kind, s5, x, w, dy)
    wi, f32 = unit_errors(r.out["out"], want, S), unit_errors(f.out["out"], want, S)
    print("MEASURED|%s|error / S (max, rms) in units of 2^-24: Winograd %.3f %.3f, f32 kernel %.3f %.3f|%.3f|%.3f"
          % (request.node.name, wi[0] / U, wi[1] / U, f32[0] / U, f32[1] / U, wi[0] / f32[0], wi[1] / f32[1]))
    assert wi[0] <= CPU_FACTOR * f32[0] and wi[1] <= CPU_FACTOR * f32[1], "Winograd %r against f32 %r" % (wi, f32)
