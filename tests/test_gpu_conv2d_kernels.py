"""Kernel-level parity of csrc/conv2d.hip (the gather-GEMM conv2d_gemm_kernel<OP, RT, CT>, its slab reduction and bias gradient)
and csrc/convkk.hip (the 5x5 LDS-halo kernel): clhip_conv2d_fwd, clhip_conv2d_bwd_data and clhip_conv2d_bwd_weight called with raw
pointers into one kernel_parity.Arena, each against the fp64 convolution of the same float32 inputs.

Dispatch.  conv_dispatch.py restates conv_ok, row_tiles, col_tiles, wgrad_splits, k_per_split, the halo kernel's shape domain and
what each call launches; conv_dispatch.CASES names for every shape and entry point the kernel, (RT, CT), the tile counts, the
splits and the w_inc / empty-split flags, and check_case_table() (run by test_conv_args_cpu.py) proves that the rows follow from
the rules and cover all seventeen reachable conv2d_gemm_kernel instantiations.  What a test can OBSERVE of that is the workspace
of the weight gradient: it starts as a NaN with a fixed payload, and with db = NULL exactly the first K*C*R*S*splits floats have
changed afterwards; an empty split's slab is all zeros.  Halo kernel versus gather-GEMM is told apart by
test_halo_kernel_and_gather_gemm_agree, which runs the halo rows through a library built with CLHIP_NO_HALO_CONV as well.

Accuracy rule, per element: |device - fp64| <= (Kd + splits + 3) * 2^-24 * S[e] + 2^-24 * |bias|, S = the same convolution of
|w| and |x| (|dy|) in fp64, Kd = C*R*S forward, K*R*S backward-data, N*OH*OW backward-weight: the forward error bound of a
Kd-term float32 dot product in any order, the split adds and the bias add; ReLU and the mask are 1-Lipschitz or exact.  Where
S[e] = 0 (dx pixels no window touches under a stride above the window; zero-weight channels) the device value must be exactly 0.
torch's float32 CPU convolution has to meet the same bound (a sanity condition on the inputs).  db (f64 partials, one rounding)
is within 1 ulp of the float32 rounding of the fp64 sum.

Every call: each operand directly between two runs of 80 NaN floats (no finite float between operand and guard), outputs and
workspace pre-filled with NaN patterns, gaps / guards / inputs unchanged afterwards (conv_parity.run_call).
test_padding_taps_at_the_ends_of_x_read_nothing singles out the taps below the last image's last rows, the only ones whose
plain address lies behind x.

Measured on one MI355X (worst element of a case over its epilogue variants: device error / bound, float32-CPU error / bound;
every check prints `MEASURED|case|what|device/bound|float32 CPU/bound` before it asserts, run with -s):
  conv2d_every_path (N,C,H,W,K,R,S,st,pad)   fwd             bwd_data        bwd_weight
  (1,5,6,6,40,3,3,1,1)              0.053 / 0.053   0.008 / 0.003   0.058 / 0.058
  (1,3,9,9,72,3,3,1,0)              0.102 / 0.102   0.005 / 0.002   0.046 / 0.046
  (1,72,7,7,72,3,3,1,1)             0.008 / 0.002   0.004 / 0.001   0.067 / 0.067
  (2,72,9,9,72,3,5,1,1)             0.003 / 0.001   0.005 / 0.001   0.030 / 0.030
  (1,3,8,8,130,3,3,1,0)             0.096 / 0.096   0.001 / 0.001   0.073 / 0.072
  (1,130,6,6,130,3,3,1,1)           0.004 / 0.002   0.003 / 0.001   0.094 / 0.094
  (2,130,9,11,130,5,3,2,2)          0.002 / 0.001   0.002 / 0.002   0.066 / 0.066
  (1,2,26,26,200,3,3,1,0)           0.197 / 0.197   0.001 / 0.001   0.004 / 0.003
  (16,2,9,25,8,3,3,1,0)             0.148 / 0.182   0.040 / 0.043   0.000 / 0.000
  (2,4,12,9,20,7,2,3,1)             0.034 / 0.041   0.006 / 0.009   0.080 / 0.053
  (3,3,35,35,64,11,11,4,2)          0.009 / 0.011   0.001 / 0.000   0.019 / 0.012
  (1,3,5,5,8,2,2,1,3)               0.188 / 0.188   0.039 / 0.031   0.017 / 0.017
  (100,4,4,5,8,3,3,1,0)             0.071 / 0.075   0.035 / 0.040   0.002 / 0.001
  (1,3,7,7,8,2,2,3,0)               0.111 / 0.123   0.030 / 0.035   0.157 / 0.157
  (2,32,13,28,96,5,5,1,2)           0.005 / 0.004   0.002 / 0.000   0.004 / 0.006      halo fwd and bwd_data
  (1,96,20,28,32,5,5,1,2)           0.002 / 0.000   0.010 / 0.003   0.004 / 0.008      halo fwd and bwd_data
  (2,64,27,27,32,5,5,1,2)           0.003 / 0.001   0.006 / 0.003   0.001 / 0.002      halo fwd and bwd_data
  (2,30,13,28,96,5,5,1,2)           0.006 / 0.004   0.001 / 0.000   0.003 / 0.005
  (1,32,6,29,32,5,5,1,2)            0.004 / 0.002   0.004 / 0.002   0.027 / 0.027
  (1,32,30,16,32,5,5,1,2)           0.005 / 0.003   0.005 / 0.003   0.009 / 0.003
  halo_kernel_and_gather_gemm_agree, the same rows through CLHIP_NO_HALO_CONV ([gemm]):
  (2,32,13,28,96,5,5,1,2)[gemm]     0.006 / 0.004   0.002 / 0.000
  (1,96,20,28,32,5,5,1,2)[gemm]     0.002 / 0.000   0.009 / 0.003
  (2,64,27,27,32,5,5,1,2)[gemm]     0.003 / 0.001   0.007 / 0.003
  operands_one_float_past_a_16_byte_boundary: bit for bit the aligned result for every operand of every case
  db: 0 ulp from the rounded fp64 sum in every case
  padding_taps_at_the_ends_of_x_read_nothing: the figures of the same rows above (worst 0.120 / 0.120, forward of (1,3,5,5,8,2,2,1,3))
  Run time on the MI355X: 81 tests in 3.3 s; 0.21 s for the first (library load), at most 0.03 s for any other.

Mutation check, run once against scratch copies of the sources (one run of this file per mutant with CLHIP_LIB on the mutant
library; each mutant stays in bounds: operands are fetched with range-checked buffer loads and every store keeps its m < M,
n < Nn guard; not part of the repository):
  (a) tab_rs built as (s << 8) | r                      38 fail: every forward / backward-data case of every_path on the gather-GEMM x34
                                                        (accuracy rule, also the R == S cases: r and s trade places), non_finite x2, misaligned x2
  (b) forward decodes tab_rs as s = rs >> 8, r = rs & 255   20 fail: every gather-GEMM forward case x17, non_finite x2, misaligned x1
  (c) wcol_rs packed as (r << 8) | s                    15 fail: every backward-weight case with pad > 0 or R != S x14 (the bounds test then
                                                        uses the wrong coordinate), misaligned x1; pad = 0 with R == S is equivalent
  (d) tm = tile % n_tiles, tn = tile / n_tiles          37 fail: every case with more than one tile x29 ("non-finite output": tiles
                                                        never written), non_finite x6, misaligned x2
  (e) an empty split returns before its store           2 fail: every_path (16,2,9,25,8,3,3,1,0) backward-weight (NaN workspace summed), non_finite x1
  (f) gather-GEMM mask uses `>= 0`                      22 fail: every gather-GEMM backward-data case x17 (0.0, -0.0 and the negative denormal,
                                                        flushed to zero by the compare, pass), non_finite x4, misaligned x1
  (g) halo kernel mask uses `>= 0`                      9 fail: the three halo backward-data rows in every_path, halo_kernel_and... x3, non_finite x2, misaligned x1
  (h) halo `ka` break one tile early                    16 fail: every halo row of every_path x6 and halo_kernel_and... x6 ("non-finite output":
      (ko0 + 32 (ka + 1) >= Cout)                       the last 32-channel tile is never stored), non_finite x2, misaligned x2
  (i) halo `ka` break removed                           not run: with Cout = 32 the second row tile would be stored 32 channels further on, into
                                                        the next image's planes; that the descriptor's range check and the other block's
                                                        stores make this harmless cannot be settled without running it.  (h) shows the tests see the break.
"""
import ctypes as C
import os

import pytest
import torch

import conv_dispatch as cd
import conv_parity as cp
from conv_parity import OUT_BITS, WS_SLACK, accuracy, check_db, check_ws, operands, reference, run_call
from kernel_parity import all_bits, bitwise_equal

pytestmark = pytest.mark.gpu

ENTRY = {"fwd": "clhip_conv2d_fwd", "bwd_data": "clhip_conv2d_bwd_data", "bwd_weight": "clhip_conv2d_bwd_weight"}
ROWS = {s: row for s, _, row in cd.CASES}


def _sid(shape):
    return "x".join(str(v) for v in shape)


# --------------------------------------------------------------------------------------------- one call
def run_conv(L, kind, shape, x, w, dy, bias=None, relu=0, relu_src=None, want_db=False, ws_floats=0, ws_bytes=None, mis=None):
    """One call of an entry point.  The output is r.out["out"] (y, dx or dw), the bias gradient r.out["db"]."""
    N, Cc, H, W, K, R, S, st, pad = shape
    OH, OW = cp.out_dims(shape)
    if kind == "fwd":
        ins, outs = [("x", x), ("w", w), ("b", bias)], [("out", N * K * OH * OW)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_fwd(p["x"], p["w"], p["b"], p["out"], *shape, int(relu), stream)
    elif kind == "bwd_data":
        ins, outs = [("dy", dy), ("w", w), ("src", relu_src)], [("out", N * Cc * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_data(p["dy"], p["w"], p["src"], p["out"], *shape, stream)
    else:
        ins, outs = [("x", x), ("dy", dy)], [("out", K * Cc * R * S), ("db", K if want_db else None), ("nodb", None if want_db else K)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_weight(p["x"], p["dy"], p["out"], p["db"], *shape, ws, nbytes, stream)
    return run_call(call, ins, outs, ws_floats=ws_floats, ws_bytes=ws_bytes, mis=mis)


def variants(kind, shape):
    """Epilogue variants of an entry point: (name, kwargs for run_conv, kwargs for accuracy)."""
    bias, src = cp.epilogue_inputs(shape)
    if kind == "fwd":
        return [("bias-relu", dict(bias=bias, relu=1), dict(bias=bias, relu=True)), ("bias", dict(bias=bias), dict(bias=bias)), ("plain", {}, {})]
    if kind == "bwd_data":
        return [("relu_src", dict(relu_src=src), dict(mask_src=src)), ("plain", {}, {})]
    return [("db", dict(want_db=True), {}), ("no-db", {}, {})]


def ws_need(kind, shape, p):
    """(floats of workspace the call is handed, floats it writes with db = NULL)."""
    if kind != "bwd_weight":
        return 0, 0
    N, Cc, H, W, K, R, S, st, pad = shape
    return cd.bwd_weight_ws_bytes(shape) // 4, K * Cc * R * S * p.splits


def check_case(case, L, kind, shape, p, mis=None, only=None):
    """Every epilogue variant of one entry point on one shape under plan p: clean arena, workspace footprint, accuracy rule, db,
    exact epilogue semantics, determinism.  Returns the outputs by variant name."""
    N, Cc, H, W, K, R, S, st, pad = shape
    M, Nn, Kd = cd.gemm_dims(kind, shape)
    x, w, dy = operands(shape)
    want, cpu, Sabs = cp.ref_of(kind, reference(shape))
    need, slabs = ws_need(kind, shape, p)
    mn = K * Cc * R * S
    outs = {}
    for name, kw, acc in variants(kind, shape):
        if only is not None and name != only:
            continue
        r = run_conv(L, kind, shape, x, w, dy, ws_floats=need + (WS_SLACK if need else 0), ws_bytes=4 * need, mis=mis, **kw)
        assert r.rc == 0 and r.clean, "%s: rc %d, gaps, guards or inputs changed: %s" % (name, r.rc, not r.clean)
        accuracy(case, name, r.out["out"], want, cpu, Sabs, Kd, p.splits, **acc)
        outs[name] = r.out["out"]
        if kind == "bwd_weight":
            if kw.get("want_db"):
                check_db(case, r.out["db"], dy)
                check_ws(r.ws, need, name, finite=False)         # slabs, then the f64 bias partials over them: nothing behind the size
            else:
                assert all_bits(r.out["nodb"], OUT_BITS), "db = NULL: the db-sized slot must keep its sentinel"
                assert all_bits(r.ws[slabs:], cp.WS_BITS), "db = NULL: workspace written behind its %d slabs" % p.splits
                assert bool(torch.isfinite(r.ws[:slabs]).all()), "a slab element of the %d promised slabs was not written" % p.splits
                live = cd.live_splits(Kd, p.splits)
                assert (live < p.splits) == p.empty
                if p.empty:
                    assert all_bits(r.ws[live * mn:slabs], 0), "an empty split's slab must be written as zeros"
            r2 = run_conv(L, kind, shape, x, w, dy, ws_floats=need + WS_SLACK, ws_bytes=4 * need, mis=mis, **kw)
            assert r2.rc == 0 and bitwise_equal(r.out["out"], r2.out["out"]), name + ": dw differs between two calls"
            if kw.get("want_db"):
                assert bitwise_equal(r.out["db"], r2.out["db"]), "db differs between two calls"
    if only is not None:
        return outs
    # exact epilogue semantics, from the variants' outputs
    if kind == "fwd":
        assert torch.equal(outs["bias-relu"], outs["bias"].clamp(min=0)), "relu is not max(v, 0) of the same v"
        OH, OW = cp.out_dims(shape)
        ch0 = outs["bias-relu"].view(N, K, OH, OW)[:, 0]
        assert all_bits(ch0, 0), "zero weights, b = -0.0, ReLU: the output must be exactly +0.0"
        assert bool((outs["bias"].view(N, K, OH, OW)[:, 0] == 0).all()) and bool((outs["plain"].view(N, K, OH, OW)[:, 0] == 0).all())
    elif kind == "bwd_data":
        src = cp.epilogue_inputs(shape)[1].reshape(-1)
        on = src > 0
        assert bitwise_equal(outs["relu_src"][on], outs["plain"][on]), "relu_src > 0 must pass the value through unchanged"
        assert all_bits(outs["relu_src"][~on], 0), "relu_src of 0.0, -0.0, a negative denormal or NaN must give exactly +0.0 (mask_src > 0 ? v : 0)"
        holes = torch.nn.grad.conv2d_input((N, Cc, H, W), torch.ones((K, Cc, R, S)), torch.ones(dy.shape), st, pad).reshape(-1) == 0
        if st > R or st > S:
            assert bool(holes.any()), "a stride above the window leaves input pixels no window touches"
        assert bool(((Sabs.reshape(-1) == 0) == holes).all())
        assert all_bits(outs["plain"][holes], 0), "dx where no window touches must be written as exactly +0.0"
    else:
        assert bitwise_equal(outs["db"], outs["no-db"]), "dw must not depend on db being asked for"
    return outs


SHAPE_KINDS = [(s, k) for s, _, _ in cd.CASES for k in cd.KINDS]


@pytest.mark.parametrize("shape,kind", SHAPE_KINDS, ids=["%s-%s" % (_sid(s), k) for s, k in SHAPE_KINDS])
def test_conv2d_every_path(request, shape, kind):
    """Every row of conv_dispatch.CASES through every epilogue variant of every entry point."""
    L = cp.product_lib()
    p = cd.plan(kind, shape)
    assert p == ROWS[shape][kind], "conv_dispatch.CASES disagrees with the restated rules"
    if kind == "bwd_weight":
        assert L.clhip_conv2d_bwd_weight_ws(*shape) == cd.bwd_weight_ws_bytes(shape)
    check_case(request.node.name, L, kind, shape, p)


# --------------------------------------------------------------------------------------------- misaligned operands
MISALIGNED = [((2, 72, 9, 9, 72, 3, 5, 1, 1), "fwd", ("x", "w", "b", "out"), "bias-relu"),
              ((2, 72, 9, 9, 72, 3, 5, 1, 1), "bwd_data", ("dy", "w", "src", "out"), "relu_src"),
              ((2, 72, 9, 9, 72, 3, 5, 1, 1), "bwd_weight", ("x", "dy", "out", "db"), "db"),
              ((2, 32, 13, 28, 96, 5, 5, 1, 2), "fwd", ("x", "w", "b", "out"), "bias-relu"),
              ((2, 32, 13, 28, 96, 5, 5, 1, 2), "bwd_data", ("dy", "w", "src", "out"), "relu_src")]


@pytest.mark.parametrize("shape,kind,names,variant", MISALIGNED, ids=["%s-%s" % (_sid(m[0]), m[1]) for m in MISALIGNED])
def test_operands_one_float_past_a_16_byte_boundary(request, shape, kind, names, variant):
    """Each operand and output in turn one float past a 16-byte boundary (gather-GEMM and halo kernel): same bits as aligned."""
    L = cp.product_lib()
    p = cd.plan(kind, shape)
    base = check_case(request.node.name, L, kind, shape, p, only=variant)[variant]
    for name in names:
        got = check_case("%s[%s]" % (request.node.name, name), L, kind, shape, p, mis=name, only=variant)[variant]
        assert bitwise_equal(got, base), "%s misaligned: the result changed" % name


# --------------------------------------------------------------------------------------------- padding taps at the tensor's ends
PAD_TAPS = [(1, 72, 7, 7, 72, 3, 3, 1, 1), (3, 3, 35, 35, 64, 11, 11, 4, 2), (1, 3, 5, 5, 8, 2, 2, 1, 3), (2, 32, 13, 28, 96, 5, 5, 1, 2)]


@pytest.mark.parametrize("shape", PAD_TAPS, ids=[_sid(s) for s in PAD_TAPS])
def test_padding_taps_at_the_ends_of_x_read_nothing(request, shape):
    """pad > 0: the taps below the last rows of the LAST image's last channel are the only ones whose plain address
    x + ((n C + c) H + h) W + w lies behind the tensor (those above the first image's first rows lie in front of it; all other
    padding taps land in a neighbouring plane, where only the accuracy rule sees them).  They reach at most pad * W + pad floats
    out, which is inside the NaN guard that touches x on either side: a kernel that loaded them would return NaN in the last
    (first) output rows.  Forward and backward-weight read x this way; gather-GEMM and halo kernel."""
    N, Cc, H, W, K, R, S, st, pad = shape
    assert 0 < pad * W + pad <= cp.GUARD
    L = cp.product_lib()
    OH, OW = cp.out_dims(shape)
    for kind, variant in (("fwd", "plain"), ("bwd_weight", "no-db")):
        out = check_case("%s[%s]" % (request.node.name, kind), L, kind, shape, cd.plan(kind, shape), only=variant)[variant]
        if kind == "fwd":
            y = out.view(N, K, OH, OW)
            assert bool(torch.isfinite(y[N - 1, :, OH - 1]).all()) and bool(torch.isfinite(y[0, :, 0]).all())


# --------------------------------------------------------------------------------------------- non-finite values stay local
LOCAL = [(1, 72, 7, 7, 72, 3, 3, 1, 1), (2, 130, 9, 11, 130, 5, 3, 2, 2), (2, 4, 12, 9, 20, 7, 2, 3, 1), (16, 2, 9, 25, 8, 3, 3, 1, 0),
         (2, 32, 13, 28, 96, 5, 5, 1, 2), (1, 96, 20, 28, 32, 5, 5, 1, 2)]


@pytest.mark.parametrize("shape", LOCAL, ids=[_sid(s) for s in LOCAL])
def test_non_finite_stays_in_its_windows(shape):
    """One NaN (then one Inf) in x at a corner and at an interior pixel of the last image: forward outputs whose window holds the
    pixel are non-finite, all others are bit for bit those of the clean run.  The same for dy in backward-data (a masked element
    under a non-finite gradient is still exactly +0.0), and for one dy element in backward-weight: exactly dw[k] and db[k]."""
    L = cp.product_lib()
    N, Cc, H, W, K, R, S, st, pad = shape
    OH, OW = cp.out_dims(shape)
    x, w, dy = operands(shape)
    need = cd.bwd_weight_ws_bytes(shape) // 4
    clean = {"fwd": run_conv(L, "fwd", shape, x, w, dy), "bwd_data": run_conv(L, "bwd_data", shape, x, w, dy),
             "bwd_weight": run_conv(L, "bwd_weight", shape, x, w, dy, want_db=True, ws_floats=need)}
    for r in clean.values():
        assert r.rc == 0 and r.clean and bool(torch.isfinite(r.out["out"]).all())
    ones_w = torch.ones((K, Cc, R, S), dtype=torch.float64)
    for val in (float("nan"), float("inf")):
        for (ph, pw), (qh, qw) in (((0, 0), (0, 0)), ((H // 2, W // 2), (OH // 2, OW // 2))):
            # forward: x[N-1][C-1][ph][pw]
            x2 = x.clone()
            x2[N - 1, Cc - 1, ph, pw] = val
            ind = torch.zeros((N, Cc, H, W), dtype=torch.float64)
            ind[N - 1, Cc - 1, ph, pw] = 1
            hit = (torch.nn.functional.conv2d(ind, ones_w, None, st, pad) != 0).reshape(-1)
            r = run_conv(L, "fwd", shape, x2, w, dy)
            assert r.rc == 0 and r.clean
            assert bool(hit.any()) or st > min(R, S)          # (a pixel no window touches: every output keeps its clean bits)
            assert bitwise_equal(r.out["out"][~hit], clean["fwd"].out["out"][~hit]), "%s in x leaked out of its windows" % val
            assert not bool(torch.isfinite(r.out["out"][hit]).any()), "%s in x did not reach all of its windows" % val
            # backward-data: dy[N-1][K-1][qh][qw]
            dy2 = dy.clone()
            dy2[N - 1, K - 1, qh, qw] = val
            ind = torch.zeros(dy.shape, dtype=torch.float64)
            ind[N - 1, K - 1, qh, qw] = 1
            hit = (torch.nn.grad.conv2d_input((N, Cc, H, W), ones_w, ind, st, pad) != 0).reshape(-1)
            r = run_conv(L, "bwd_data", shape, x, w, dy2)
            assert r.rc == 0 and r.clean and bool(hit.any())
            assert bitwise_equal(r.out["out"][~hit], clean["bwd_data"].out["out"][~hit]), "%s in dy leaked out of its windows" % val
            assert not bool(torch.isfinite(r.out["out"][hit]).any()), "%s in dy did not reach all of its windows" % val
            src = torch.ones((N, Cc, H, W)).reshape(-1)
            first = int(torch.nonzero(hit)[0])
            src[first] = 0.0
            rm = run_conv(L, "bwd_data", shape, x, w, dy2, relu_src=src.view(N, Cc, H, W))
            assert rm.rc == 0 and rm.clean and all_bits(rm.out["out"][first:first + 1], 0), "a masked element is +0.0 whatever lies under it"
            keep = torch.ones(hit.numel(), dtype=torch.bool)
            keep[first] = False
            assert bitwise_equal(rm.out["out"][keep], r.out["out"][keep])
        # backward-weight: one dy element of out-channel K-1 at an interior pixel whose window lies inside the map where it can
        dy2 = dy.clone()
        dy2[N - 1, K - 1, OH // 2, OW // 2] = val
        r = run_conv(L, "bwd_weight", shape, x, w, dy2, want_db=True, ws_floats=need)
        assert r.rc == 0 and r.clean
        dw, dw0 = r.out["out"].view(K, -1), clean["bwd_weight"].out["out"].view(K, -1)
        assert bitwise_equal(dw[:K - 1], dw0[:K - 1]) and bitwise_equal(r.out["db"][:K - 1], clean["bwd_weight"].out["db"][:K - 1]), \
            "%s in dy[.., K-1, ..] leaked into another out-channel" % val
        inside = torch.nn.grad.conv2d_weight(torch.ones((N, Cc, H, W), dtype=torch.float64), (K, Cc, R, S),
                                             (dy2 != dy).double(), st, pad)[K - 1].reshape(-1) != 0       # taps that meet a map pixel
        assert not bool(torch.isfinite(dw[K - 1][inside]).any()) and not bool(torch.isfinite(r.out["db"][K - 1:]).any()), \
            "%s in dy[.., K-1, ..] did not reach dw[K-1] and db[K-1]" % val


# --------------------------------------------------------------------------------------------- halo kernel against gather-GEMM
@pytest.fixture(scope="module")
def nohalo_lib():
    """libclhip_nohalo.so: conv2d.hip compiled with CLHIP_NO_HALO_CONV (halo_kernel() false: every shape on the gather-GEMM), loaded
    next to the product library.  Rebuilt when the fingerprint of conv2d.hip, the headers and the flags changes; a build that
    fails is an error of these tests, not a reason to skip them."""
    import glob
    from clsurvey_amd import _lib, build
    L = _lib.lib()                                   # maps torch's HIP runtime first (see _lib.lib)
    out = os.path.join(build.HERE, "libclhip_nohalo.so")
    stamp = out + ".sha256"
    hdrs = sorted(glob.glob(os.path.join(build.CSRC, "*.hpp"))) + [os.path.join(build.HERE, "..", "include", "clhip.h")]
    want = build._fingerprint([os.path.join(build.CSRC, "conv2d.hip")] + hdrs, build.FLAGS + ["-DCLHIP_NO_HALO_CONV"])
    have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(out) else ""
    if have != want:
        assert build.build_variant("nohalo", "conv2d.hip", ["CLHIP_NO_HALO_CONV"], verbose=False) == out
        with open(stamp, "w") as f:
            f.write(want + "\n")
    h = C.CDLL(os.path.abspath(out))
    for name in list(ENTRY.values()) + ["clhip_conv2d_bwd_weight_ws"]:
        fn, src = getattr(h, name), getattr(L, name)
        fn.restype, fn.argtypes = src.restype, src.argtypes
    return h


HALO = cd.halo_cases()


@pytest.mark.parametrize("shape,kind", HALO, ids=["%s-%s" % (_sid(s), k) for s, k in HALO])
def test_halo_kernel_and_gather_gemm_agree(request, nohalo_lib, shape, kind):
    """Every halo row through the product library (convkk_kernel) and through a library whose halo_kernel() is false (the
    gather-GEMM instantiation conv_dispatch.plan(halo=False) names): both meet the accuracy rule with identical epilogue semantics.
    That two DIFFERENT kernels ran shows in the bits: the halo kernel sums in-channel pairs with the taps inside, the gather-GEMM
    runs over (channel, tap) in chunks of 32, so among thousands of outputs some must round differently.  Which library ran which
    kernel is not observable from results; that rests on conv_dispatch and on mutants (g) and (h), which only the halo rows see."""
    assert cd.plan(kind, shape).kernel == cd.HALO
    pg = cd.plan(kind, shape, halo=False)
    assert pg.kernel == cd.G
    a = check_case(request.node.name + "[halo]", cp.product_lib(), kind, shape, cd.plan(kind, shape))
    b = check_case(request.node.name + "[gemm]", nohalo_lib, kind, shape, pg)
    assert not bitwise_equal(a["plain"], b["plain"]), "bit for bit the same result: the two libraries ran the same kernel"
    if kind == "bwd_data":
        assert bool(((a["relu_src"] == 0) == (b["relu_src"] == 0)).all()), "the two kernels mask different elements"
