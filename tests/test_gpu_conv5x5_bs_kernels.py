"""Kernel-level parity of the bf16-split 5x5 kernels: clhip_conv5x5_bs_fwd / clhip_conv5x5_bs_bwd_data (the 25-tap instantiations
BsGeo<16,8,..,5> and BsGeo<32,4,..,5> of csrc/bsconv.hip and the weight image they build) and clhip_conv5x5_bs_bwd_weight
(bs_wgradk_kernel<5,1> of csrc/bswgrad5.hip and its slab reduction), called with raw pointers into one kernel_parity.Arena, each
against the fp64 convolution of the same float32 inputs.

Dispatch.  conv_dispatch.py restates clhip_internal_bs_ok, the W > 16 geometry choice, clhip_internal_bs5_ws and bsk_ok<5> /
bsk_splits<5> / bsk_ws<5>; BS5_CASES and BSK5_CASES carry the shapes (geometry switch at W = 16 / 17, the minima H = 4, W = 9 and
W = 8, one-row and one-column tails, nine pixel blocks across the 8-block XCD group, 102 shares over 108 rows).  Observable:
forward / backward-data write exactly the weight image (clhip_internal_bs5_ws bytes) into the NaN workspace, the weight gradient
exactly splits * (25 K C + K) floats.  bs_conv_body has three epilogues (conv_dispatch.bs5_epilogue): odd maps store lane by
lane, even maps with W % 4 == 0 store whole float4 row pieces and load the mask as float4, other even maps store and load
float2.  The six rows of the issue are all odd; (2,64,64,8,20), (1,64,64,4,12) (float4, both geometries) and (1,64,64,6,18)
(float2) run the other two, aligned and with output, mask and inputs 1 and 2 floats off a 16-byte boundary.

Accuracy rule, per element: |device - fp64| <= ((Kd + splits + 3) * 2^-24 + 2^-26) * S[e] + 2^-24 * |bias| — the any-order float32
dot-product bound of test_gpu_conv2d_kernels.py plus the header's bound for the three piece products the kernels drop; Kd = 25 C
forward, 25 K backward-data, N*H*W backward-weight.  No case exceeds it (the fallback of 4 x the f32 sibling's error is not needed).
db of the weight gradient: any-order bound (N*H*W + splits + 3) * 2^-24 * sum|dy|.

Measured on one MI355X (device error / bound, float32-CPU error / bound, worst over the epilogue variants; run with -s):
  bs5_conv_every_geometry (N,C,K,H,W)   fwd             bwd_data
  (1,32,64,4,9)                 0.001 / 0.003   ENOTSUP
  (2,64,64,9,16)                0.001 / 0.001   0.001 / 0.001
  (1,64,128,5,17)               0.001 / 0.001   0.000 / 0.000
  (1,96,64,4,33)                0.001 / 0.000   ENOTSUP
  (3,64,96,7,27)                ENOTSUP         0.001 / 0.000
  (9,64,64,4,9)                 0.001 / 0.001   0.001 / 0.001
  (2,64,64,8,20)                0.001 / 0.001   0.001 / 0.001      float4 epilogue, 32-wide geometry
  (1,64,64,4,12)                0.001 / 0.001   0.001 / 0.001      float4 epilogue, 16-wide geometry
  (1,64,64,6,18)                0.001 / 0.001   0.001 / 0.001      float2 epilogue
  bs5_outputs_off_a_16_byte_boundary: (3,64,96,7,27) bwd_data, (1,96,64,4,33) fwd, (1,64,64,7,27) fwd (scalar stores) and
  (2,64,64,8,20), (1,64,64,4,12) (float4), (1,64,64,6,18) (float2), forward and backward-data each — bit for bit the aligned
  result with the output, the mask / bias and each input 1 and 2 floats off
  bs5_weight_gradient_operands_off_a_16_byte_boundary: (1,64,32,6,27), x, dy, dw, db 1 and 2 floats off — bit for bit the aligned result
  bs5_weight_gradient_every_shape     dw              db error in units of 2^-24 sum|dy|: this kernel (fp32 running sums per lane,
                                                      fp32 slabs) | clhip_conv2d_bwd_weight (f64 partials, one rounding) on the same dy
  (1,32,32,1,8)                 0.107 / 0.302   0.836 | 0.459
  (2,32,64,3,9)                 0.024 / 0.042   0.422 | 0.172
  (1,64,32,6,27)                0.004 / 0.023   0.302 | 0.123
  (3,32,32,2,33)                0.003 / 0.008   0.156 | 0.097
  (2,64,64,27,27)               0.000 / 0.003   0.070 | 0.039
  (the fp32 bias partials cost about a factor 2 at these sizes, far inside the any-order bound of N*H*W + splits + 3 units)
  bs5_error_is_that_of_an_fp32_chain, all-positive operands, error / S in units of 2^-24 (max, rms): bf16-split | f32 kernel
  (2,64,64,9,16) fwd            13.5  3.18 | 40.0  8.72       ratio 0.34 0.37
  (1,64,128,5,17) fwd           12.6  2.95 | 37.7  8.26       ratio 0.33 0.36
  (2,64,64,9,16) bwd_data       14.5  3.22 | 37.6  8.86       ratio 0.38 0.36
  (3,64,96,7,27) bwd_data       19.4  3.88 | 45.5  10.8       ratio 0.43 0.36
  (1,64,32,6,27) bwd_weight     1.58  0.48 | 12.5  2.78       ratio 0.13 0.17
  (2,64,64,27,27) bwd_weight    0.98  0.36 | 9.62  1.99       ratio 0.10 0.18
  Run time on the MI355X: 40 tests in 3.5 s; 0.46 s for the largest weight gradient, 0.28 s for the first test (library load),
  at most 0.13 s for any other.

Mutation check, run once against scratch copies of the sources (one run of this file per mutant with CLHIP_LIB on the mutant
library; loads are range-checked buffer loads and no store index changes, so each stays in bounds; not part of the repository):
  (a) bswgrad5.hip: nd = min(8, max(0, W - col0 + 1))     7 fail: weight_gradient_every_shape x5 (the column behind the map's edge — the next
      (one pixel more than the map has, in split_d too)    row's first pixel — enters dw and db), error_is_that_of_an_fp32_chain x2 (bwd_weight)
  (b) bsconv.hip: `mask_src[o] >= 0.f` for the window's    5 fail: every backward-data case of conv_every_geometry x4 (accuracy rule, 600x to
      first pixel (the epilogue of odd maps)               2900x the bound), outputs_off_a_16_byte_boundary x1
  (b4) bsconv.hip: `ms.x >= 0.f` in the float4 epilogue    4 fail: conv_every_geometry (2,64,64,8,20) and (1,64,64,4,12) backward-data,
                                                           outputs_off_a_16_byte_boundary on the same two
  (b2) bsconv.hip: `m0.x >= 0.f` in the float2 epilogue    2 fail: conv_every_geometry (1,64,64,6,18) backward-data, outputs_off... on the same
  (c) bs_launch5: `W >= 16` picks the 32-wide geometry    none fails, and none can: EQUIVALENT.  An output pixel's sum runs over the same
                                                           chunks, taps and piece products in the same order in either geometry (the comment
                                                           above bs_conv_mixed_kernel), so W = 16 gives the same bits in BsGeo<32,4,..,5>
                                                           with half of each block idle; only the grid differs, which no result shows.
"""
import pytest
import torch

import conv_dispatch as cd
import conv_parity as cp
from conv_parity import OUT_BITS, U, WS_SLACK, accuracy, check_ws, operands, reference, run_call, unit_errors
from kernel_parity import all_bits, bitwise_equal

pytestmark = pytest.mark.gpu

ENOTSUP = -3
DROPPED = 2.0 ** -26          # the three piece products a1 b2, a2 b1, a2 b2 the kernels leave out (header of bsconv.hip)


def full(s5):
    """(N, C, K, H, W) -> the (N, C, H, W, K, R, S, stride, pad) of conv_dispatch / conv_parity."""
    N, Cc, K, H, W = s5
    return (N, Cc, H, W, K, 5, 5, 1, 2)


def _sid(s5):
    return "x".join(str(v) for v in s5)


def run_bs(L, kind, s5, x, w, dy, bias=None, relu=0, relu_src=None, want_db=False, ws_floats=0, ws_bytes=None, mis=None, mis_by=1):
    N, Cc, K, H, W = s5
    if kind == "fwd":
        ins, outs = [("x", x), ("w", w), ("b", bias)], [("out", N * K * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv5x5_bs_fwd(p["x"], p["w"], p["b"], p["out"], N, Cc, K, H, W, int(relu), ws, nbytes, stream)
    elif kind == "bwd_data":
        ins, outs = [("dy", dy), ("w", w), ("src", relu_src)], [("out", N * Cc * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv5x5_bs_bwd_data(p["dy"], p["w"], p["src"], p["out"], N, Cc, K, H, W, ws, nbytes, stream)
    else:
        ins, outs = [("x", x), ("dy", dy)], [("out", K * Cc * 25), ("db", K if want_db else None), ("nodb", None if want_db else K)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv5x5_bs_bwd_weight(p["x"], p["dy"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    return run_call(call, ins, outs, ws_floats=ws_floats, ws_bytes=ws_bytes, mis=mis, mis_by=mis_by)


def run_f32(L, kind, s5, x, w, dy, want_db=False):
    """The f32 sibling of the same operator on the same data: clhip_conv2d_fwd / _bwd_data / _bwd_weight."""
    shape = full(s5)
    N, Cc, K, H, W = s5
    need = cd.bwd_weight_ws_bytes(shape) // 4
    if kind == "fwd":
        ins, outs = [("x", x), ("w", w)], [("out", N * K * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_fwd(p["x"], p["w"], None, p["out"], *shape, 0, stream)
    elif kind == "bwd_data":
        ins, outs = [("dy", dy), ("w", w)], [("out", N * Cc * H * W)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_data(p["dy"], p["w"], None, p["out"], *shape, stream)
    else:
        ins, outs = [("x", x), ("dy", dy)], [("out", K * Cc * 25), ("db", K if want_db else None)]

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_weight(p["x"], p["dy"], p["out"], p["db"], *shape, ws, nbytes, stream)
    r = run_call(call, ins, outs, ws_floats=need)
    assert r.rc == 0 and r.clean
    return r


def image_floats(kind, s5):
    N, Cc, K, H, W = s5
    return (cd.bs5_image_bytes(Cc, K) if kind == "fwd" else cd.bs5_image_bytes(K, Cc)) // 4


def check_conv(case, L, kind, s5, mis=None, mis_by=1, only=None):
    """Forward or backward-data, every epilogue variant: clean arena, exactly the weight image written, accuracy rule, exact
    epilogue semantics.  Returns the outputs by variant name."""
    N, Cc, K, H, W = s5
    shape = full(s5)
    x, w, dy = operands(shape)
    want, cpu, Sabs = cp.ref_of(kind, reference(shape))
    bias, src = cp.epilogue_inputs(shape)
    Kd = 25 * (Cc if kind == "fwd" else K)
    img = image_floats(kind, s5)
    if kind == "fwd":
        vs = [("bias-relu", dict(bias=bias, relu=1), dict(bias=bias, relu=True)), ("bias", dict(bias=bias), dict(bias=bias)), ("plain", {}, {})]
    else:
        vs = [("relu_src", dict(relu_src=src), dict(mask_src=src)), ("plain", {}, {})]
    outs = {}
    for name, kw, acc in vs:
        if only is not None and name != only:
            continue
        r = run_bs(L, kind, s5, x, w, dy, ws_floats=img + WS_SLACK, ws_bytes=4 * img, mis=mis, mis_by=mis_by, **kw)
        assert r.rc == 0 and r.clean, "%s: rc %d, gaps, guards or inputs changed: %s" % (name, r.rc, not r.clean)
        check_ws(r.ws, img, name, finite=False)
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


CONV = [(s, k) for s, _, _, _ in cd.BS5_CASES for k in ("fwd", "bwd_data")]


@pytest.mark.parametrize("s5,kind", CONV, ids=["%s-%s" % (_sid(s), k) for s, k in CONV])
def test_bs5_conv_every_geometry(request, s5, kind):
    """Every row of conv_dispatch.BS5_CASES: the entry point the row excludes answers CLHIP_ENOTSUP and writes nothing."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    row = [r for r in cd.BS5_CASES if r[0] == s5][0]
    assert cd.bs5_geometry(H, W) == row[2] and L.clhip_conv5x5_bs_ws(Cc, K) == cd.bs5_ws_bytes(Cc, K)
    if kind not in row[1]:
        assert not cd.bs5_ok(kind, *s5)
        x, w, dy = operands(full(s5))
        r = run_bs(L, kind, s5, x, w, dy, ws_floats=cd.bs5_ws_bytes(Cc, K) // 4)
        assert r.rc == ENOTSUP and r.clean and all_bits(r.out["out"], OUT_BITS) and all_bits(r.ws, cp.WS_BITS)
        return
    assert cd.bs5_ok(kind, *s5)
    check_conv(request.node.name, L, kind, s5)


MISALIGNED = [((3, 64, 96, 7, 27), "bwd_data", "relu_src"), ((1, 96, 64, 4, 33), "fwd", "bias-relu"), ((1, 64, 64, 7, 27), "fwd", "bias-relu"),
              ((2, 64, 64, 8, 20), "bwd_data", "relu_src"), ((2, 64, 64, 8, 20), "fwd", "bias-relu"), ((1, 64, 64, 4, 12), "bwd_data", "relu_src"),
              ((1, 64, 64, 4, 12), "fwd", "bias-relu"), ((1, 64, 64, 6, 18), "bwd_data", "relu_src"), ((1, 64, 64, 6, 18), "fwd", "bias-relu")]
EPILOGUES = {(3, 64, 96, 7, 27): "scalar", (1, 96, 64, 4, 33): "scalar", (1, 64, 64, 7, 27): "scalar", (2, 64, 64, 8, 20): "float4",
             (1, 64, 64, 4, 12): "float4", (1, 64, 64, 6, 18): "float2"}


@pytest.mark.parametrize("s5,kind,variant", MISALIGNED, ids=["%s-%s" % (_sid(m[0]), m[1]) for m in MISALIGNED])
def test_bs5_outputs_off_a_16_byte_boundary(request, s5, kind, variant):
    """The output, the mask of backward-data / the bias, then each input one float and two floats past a 16-byte boundary: at
    W = 27 and W = 33 (scalar stores), at W = 20 and W = 12 (float4 row stores and float4 mask loads, both geometries) and at
    W = 18 (float2 stores and mask loads) — same bits as aligned, nothing written outside the output."""
    L = cp.product_lib()
    assert cd.bs5_epilogue(s5[3], s5[4]) == EPILOGUES[s5]
    base = check_conv(request.node.name, L, kind, s5, only=variant)[variant]
    names = ("out", "src", "dy", "w") if kind == "bwd_data" else ("out", "b", "x", "w")
    for name in names:
        for by in (1, 2):
            got = check_conv("%s[%s+%d]" % (request.node.name, name, by), L, kind, s5, mis=name, mis_by=by, only=variant)[variant]
            assert bitwise_equal(got, base), "%s %d floats off: the result changed" % (name, by)


# --------------------------------------------------------------------------------------------- weight gradient
WG = [s for s, _, _ in cd.BSK5_CASES]


@pytest.mark.parametrize("s5", WG, ids=[_sid(s) for s in WG])
def test_bs5_weight_gradient_every_shape(request, s5):
    """dw per element, db against the any-order bound and next to the f64-accumulated db of clhip_conv2d_bwd_weight, exactly
    splits * (25 K C + K) floats of workspace, bitwise determinism, db = NULL."""
    L = cp.product_lib()
    case = request.node.name
    N, Cc, K, H, W = s5
    shape = full(s5)
    splits = cd.bsk5_splits(*s5)
    assert splits == [r for r in cd.BSK5_CASES if r[0] == s5][0][1]
    need = cd.bsk5_ws_bytes(*s5) // 4
    assert need == splits * (25 * K * Cc + K) and L.clhip_conv5x5_bs_bwd_weight_ws(*s5) == 4 * need
    x, w, dy = operands(shape)
    ref = reference(shape)
    Kd = N * H * W
    outs = {}
    for name, want_db in (("db", True), ("no-db", False)):
        r = run_bs(L, "bwd_weight", s5, x, w, dy, want_db=want_db, ws_floats=need + WS_SLACK, ws_bytes=4 * need)
        assert r.rc == 0 and r.clean, "%s: rc %d, gaps, guards or inputs changed: %s" % (name, r.rc, not r.clean)
        check_ws(r.ws, need, name)
        accuracy(case, name, r.out["out"], ref.dw64, ref.dw32, ref.s_dw, Kd, splits, extra=DROPPED)
        r2 = run_bs(L, "bwd_weight", s5, x, w, dy, want_db=want_db, ws_floats=need + WS_SLACK, ws_bytes=4 * need)
        assert r2.rc == 0 and bitwise_equal(r.out["out"], r2.out["out"]), "dw differs between two calls"
        outs[name] = r.out["out"]
        if want_db:
            assert bitwise_equal(r.out["db"], r2.out["db"]), "db differs between two calls"
            f32 = run_f32(L, "bwd_weight", s5, x, w, dy, want_db=True)
            unit = U * ref.s_db
            e_bs = float(((r.out["db"].double() - ref.db64).abs() / unit).max())
            e_f32 = float(((f32.out["db"].double() - ref.db64).abs() / unit).max())
            print("MEASURED|%s|db error / (2^-24 sum|dy|): bf16-split kernel (fp32 partial sums), clhip_conv2d_bwd_weight (f64)|%.3f|%.3f" % (case, e_bs, e_f32))
            assert bool(torch.isfinite(r.out["db"]).all()) and e_bs <= Kd + splits + 3, "db: %.3f units, bound %d" % (e_bs, Kd + splits + 3)
            assert e_f32 <= 1.0, "the f64-accumulated db is one rounding: at most 2^-24 |db| <= 2^-24 sum|dy|"
        else:
            assert all_bits(r.out["nodb"], OUT_BITS), "db = NULL: the db-sized slot must keep its sentinel"
    assert bitwise_equal(outs["db"], outs["no-db"]), "dw must not depend on db being asked for"


def test_bs5_weight_gradient_operands_off_a_16_byte_boundary(request):
    """x, dy, dw and db in turn one and two floats past a 16-byte boundary at W = 27 (the kernel loads 16 bytes at whatever 4-byte
    offset a row starts): same bits as aligned."""
    L = cp.product_lib()
    s5 = (1, 64, 32, 6, 27)
    N, Cc, K, H, W = s5
    shape = full(s5)
    splits, need = cd.bsk5_splits(*s5), cd.bsk5_ws_bytes(*s5) // 4
    x, w, dy = operands(shape)
    ref = reference(shape)
    base = run_bs(L, "bwd_weight", s5, x, w, dy, want_db=True, ws_floats=need + WS_SLACK, ws_bytes=4 * need)
    assert base.rc == 0 and base.clean
    for name in ("x", "dy", "out", "db"):
        for by in (1, 2):
            r = run_bs(L, "bwd_weight", s5, x, w, dy, want_db=True, ws_floats=need + WS_SLACK, ws_bytes=4 * need, mis=name, mis_by=by)
            assert r.rc == 0 and r.clean, "%s %d floats off: rc %d, gaps, guards or inputs changed" % (name, by, r.rc)
            check_ws(r.ws, need, name)
            accuracy("%s[%s+%d]" % (request.node.name, name, by), "db", r.out["out"], ref.dw64, ref.dw32, ref.s_dw, N * H * W, splits, extra=DROPPED)
            assert bitwise_equal(r.out["out"], base.out["out"]) and bitwise_equal(r.out["db"], base.out["db"]), \
                "%s %d floats off: the result changed" % (name, by)


# --------------------------------------------------------------------------------------------- coherent errors
COHERENT = [("fwd", (2, 64, 64, 9, 16)), ("fwd", (1, 64, 128, 5, 17)), ("bwd_data", (2, 64, 64, 9, 16)), ("bwd_data", (3, 64, 96, 7, 27)),
            ("bwd_weight", (1, 64, 32, 6, 27)), ("bwd_weight", (2, 64, 64, 27, 27))]


@pytest.mark.parametrize("kind,s5", COHERENT, ids=["%s-%s" % (_sid(s), k) for k, s in COHERENT])
def test_bs5_error_is_that_of_an_fp32_chain(request, kind, s5):
    """All-positive operands: dropped-term and truncation errors add up instead of cancelling.  In units of S[e] (max and rms) the
    bf16-split kernel's error must not exceed 2 x that of the f32 kernel of the same operator on the same data."""
    L = cp.product_lib()
    shape = full(s5)
    N, Cc, K, H, W = s5
    x, w, dy = operands(shape, positive=True)
    want, cpu, Sabs = cp.ref_of(kind, reference(shape, positive=True))
    ws = cd.bsk5_ws_bytes(*s5) // 4 if kind == "bwd_weight" else image_floats(kind, s5)
    r = run_bs(L, kind, s5, x, w, dy, ws_floats=ws)
    assert r.rc == 0 and r.clean
    f = run_f32(L, kind, s5, x, w, dy)
    bs, f32 = unit_errors(r.out["out"], want, Sabs), unit_errors(f.out["out"], want, Sabs)
    print("MEASURED|%s|error / S (max, rms) in units of 2^-24: bf16-split %.3f %.3f, f32 kernel %.3f %.3f|%.3f|%.3f"
          % (request.node.name, bs[0] / U, bs[1] / U, f32[0] / U, f32[1] / U, bs[0] / f32[0], bs[1] / f32[1]))
    assert bool(torch.isfinite(r.out["out"]).all())
    assert bs[0] <= 2 * f32[0] and bs[1] <= 2 * f32[1], "bf16-split %r against f32 %r" % (bs, f32)


# --------------------------------------------------------------------------------------------- non-finite values stay local
def test_bs5_non_finite_stays_in_its_windows():
    """One NaN, then one Inf: in x (forward) and dy (backward-data) at a corner and an interior pixel of the last image — outputs
    whose 5x5 window holds the pixel are non-finite, all others bit for bit those of the clean run; in one dy element of the weight
    gradient — exactly dw[k] and db[k]."""
    L = cp.product_lib()
    s5 = (2, 64, 64, 9, 16)
    N, Cc, K, H, W = s5
    shape = full(s5)
    x, w, dy = operands(shape)
    img = cd.bs5_ws_bytes(Cc, K) // 4
    need = cd.bsk5_ws_bytes(*s5) // 4
    clean = {"fwd": run_bs(L, "fwd", s5, x, w, dy, ws_floats=img), "bwd_data": run_bs(L, "bwd_data", s5, x, w, dy, ws_floats=img),
             "bwd_weight": run_bs(L, "bwd_weight", s5, x, w, dy, want_db=True, ws_floats=need)}
    for r in clean.values():
        assert r.rc == 0 and r.clean and bool(torch.isfinite(r.out["out"]).all())
    for val in (float("nan"), float("inf")):
        for ph, pw in ((0, 0), (H // 2, W // 2), (H - 1, W - 1)):
            for kind, ch in (("fwd", Cc), ("bwd_data", K)):
                x2, dy2 = x.clone(), dy.clone()
                (x2 if kind == "fwd" else dy2)[N - 1, ch - 1, ph, pw] = val
                hit = torch.zeros((N, 1, H, W), dtype=torch.bool)
                hit[N - 1, 0, max(ph - 2, 0):ph + 3, max(pw - 2, 0):pw + 3] = True
                hit = hit.expand(N, K if kind == "fwd" else Cc, H, W).reshape(-1)
                r = run_bs(L, kind, s5, x2, w, dy2, ws_floats=img)
                assert r.rc == 0 and r.clean
                assert bitwise_equal(r.out["out"][~hit], clean[kind].out["out"][~hit]), "%s leaked out of its windows (%s)" % (val, kind)
                assert not bool(torch.isfinite(r.out["out"][hit]).any()), "%s did not reach all of its windows (%s)" % (val, kind)
        dy2 = dy.clone()
        dy2[N - 1, K - 1, H // 2, W // 2] = val                    # rows H/2 - 2 .. H/2 + 2 and columns W/2 - 2 .. W/2 + 2 lie inside the map
        r = run_bs(L, "bwd_weight", s5, x, w, dy2, want_db=True, ws_floats=need)
        assert r.rc == 0 and r.clean
        dw, dw0 = r.out["out"].view(K, -1), clean["bwd_weight"].out["out"].view(K, -1)
        assert bitwise_equal(dw[:K - 1], dw0[:K - 1]) and bitwise_equal(r.out["db"][:K - 1], clean["bwd_weight"].out["db"][:K - 1]), \
            "%s in dy[.., K-1, ..] leaked into another out-channel" % val
        assert not bool(torch.isfinite(dw[K - 1]).any()) and not bool(torch.isfinite(r.out["db"][K - 1:]).any()), \
            "%s in dy[.., K-1, ..] did not reach all of dw[K-1] and db[K-1]" % val
