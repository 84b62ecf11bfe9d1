"""Kernel-level parity of the direct f32 3x3 kernels of csrc/conv3x3.hip and csrc/conv3x3_wgrad.hip: clhip_conv3x3_fwd /
_relu_pool_fwd / _bwd_data / _bwd_data_unpool (conv3x3_mfma_kernel, _mixed_kernel, _mixed2_kernel, conv3x3_c3_relu_pool_kernel,
conv3x3_c3w64_relu_pool_kernel) and clhip_conv3x3_bwd_weight / _unpool / _slabs / _reduce (conv3x3_wgrad_kernel,
conv3x3_wgrad_smallc_kernel, conv3x3_wgrad_c3_unpool_kernel, wgrad_reduce_kernel), called with raw pointers into one
kernel_parity.Arena (arg-max codes: a ByteArena beside it), each against the fp64 convolution of the same float32 inputs.

Dispatch.  conv3x3_dispatch.py restates vec_ok, launch_conv, the first-layer choice, make_plan and the kernel choice of
bwd_weight_impl; FWD_CASES, POOL_CASES and WG_CASES carry one hand-worked row per arm (test_conv3x3_args_cpu.py checks the tables
without a GPU).  Every forward row runs forward on the layer (C, K) = (Cin, Cout) and backward-data on (C, K) = (Cout, Cin).
Observable: forward / backward-data leave the workspace sentinel alone; the weight gradient writes exactly splits * (9 K C + K)
floats — the `groups` slabs that clhip_conv3x3_bwd_weight_ws adds are never touched.

Accuracy rule, per element: |device - fp64| <= (Kd + splits + 3) * 2^-24 * S[e] + 2^-24 |bias|, S the same product of absolute values.
Roundings on the path of one term, read from the kernels:
  chunked kernel (forward, backward-data)   every output element is ONE v_mfma_f32_32x32x2 chain over (chunk, channel pair, tap): 9 Cin
      products, each added to the accumulator once (padding and the channel tail add exact zeros): Kd = 9 Cin, splits = 0; the bias is
      one more addition behind the chain (bias_s), ReLU and the mask are exact.
  first-layer kernels (c3, c3w64)           14 k-pairs = 27 taps + one zero slot on one accumulator: Kd = 27; the bias is added behind
      the chain (the 28th slot carries A = 0, not the bias), one rounding.
  weight gradient                           a block's share of the N H W pixels chained on one accumulator per tap (conv3x3_wgrad_kernel),
      in the pixel-split form four wave partials added through LDS (3 more), in the first-layer kernels two halves (1 more); the
      slabs are summed in f64 and rounded once: Kd = N H W, `splits` and the + 3 cover the partial sums' roundings.
  db                                        every kernel sums dy in f64 per block and rounds the block's sum to float32 once (smallc / c3_unpool:
      the half sums once more), the reduction sums the slabs in f64 and rounds once: |db - fp64| <= 3 * 2^-24 * sum|dy| whatever
      `splits` is (the slab roundings are relative to disjoint parts of sum|dy|).  conv_parity.check_db's 1 ulp of the rounded fp64
      sum holds for a kernel whose partials stay f64 to the end (clhip_conv2d_bwd_weight); here every slab carries its share as a
      float32, so db is a sum of float32 partials and the bound of such a sum is what is asserted — 3 units, far inside the any-order
      (N H W + splits + 3).  The distance in ulp of db is printed: 2 - 806 on these rows (sum dy cancels to ~ sqrt(N H W) of sum|dy|).
torch's float32 CPU convolution must meet the same bounds (conv_parity.accuracy).

Exact properties.  Out-channel 0 has zero weights and bias[0] = -0.0: the chain adds (+-0) to +0.0 and stays +0.0, (+0.0) + (-0.0) =
+0.0, max(+0.0, 0) = +0.0: every forward variant gives +0.0 bits there; the pooled kernels give +0.0 with code 4.  A masked
backward-data element is the literal 0.f.  Fused pooling on the chunked kernel: `pool_idx` is a run-time argument of one instantiation
and changes only which lane holds which pixel (tile_pixel) — a pixel's sum is the same chain over (chunk, pair, tap) in any lane, so the
pooled value is bit for bit the window maximum of clhip_conv3x3_fwd(relu = 1).  The same argument makes every image of a mixed launch
equal to the one-geometry launch's (the dense 13 x 13 tile has no such partner: the rule alone).  Un-pooling:
the 16-byte staging writes (code == position ? dy : 0.f) into the LDS plane where the dense form writes the dense dy's element, which
torch_ref.unpool builds as the same value or +0.0; everything behind the plane is the same code: bit for bit, for backward-data, the
general weight gradient and the first-layer kernel with codes.  conv3x3_wgrad_c3_unpool_kernel is another kernel with another order:
the rule alone.  Scalar staging fills the same LDS planes as the 16-byte staging: bit for bit (forward, backward-data, weight gradient).

Found and fixed with these tests and test_conv3x3_args_cpu.py: see there (index-width limits; the odd-map refusal of the bf16-split
entry points, which on the parent library wrote the weight image into the workspace before answering CLHIP_ENOTSUP).  Also:
clhip_conv3x3_relu_pool_fwd sent C = 3, W % 32 == 0 to conv3x3_c3_relu_pool_kernel whatever the addresses of y_pool and the codes,
which that kernel stores 16 bytes at a time; other addresses are now routed to the chunked kernel (read from the code, not provoked; no
call is refused).  The same for the slab reduction: wgrad_reduce_block loaded 16 bytes at a time whenever the slab size was a multiple of 4,
whatever the address of the slabs, which clhip_conv3x3_bwd_weight_reduce takes from its caller; off a 16-byte boundary it now takes its
scalar loads — the same order per element, the same bits (test_reduce_of_one_slab_copies_it).

Measured on one MI355X (device error / bound | float32-CPU error / bound, worst over the variants of a test; run with -s):
  conv_every_geometry (N,Cin,Cout,H,W)  arm                      fwd             bwd_data
  (300,8,64,4,32)             mixed<32,4,2>            0.073 | 0.070   0.078 | 0.072
  (256,8,64,4,32)             (32,2,1) 16-byte         0.079 | 0.082   0.074 | 0.084
  (512,8,64,4,32)             (32,4,1) 16-byte         0.072 | 0.093   0.076 | 0.072
  (130,8,256,8,16)            mixed2<16,8,1,4,1>       0.081 | 0.079   0.073 | 0.077
  (260,8,256,8,8)             mixed2<8,8,2,8,1>        0.086 | 0.079   0.079 | 0.070
  (261,8,256,8,8)             (8,8,2) 16-byte          0.079 | 0.079   0.077 | 0.068
  (2,16,72,4,32)              (32,2,1) 16-byte         0.025 | 0.026   0.022 | 0.030
  (225,8,72,4,32)             (32,4,1) 16-byte         0.077 | 0.076   0.071 | 0.069
  (2,16,72,8,16)              (16,4,1) 16-byte         0.022 | 0.025   0.022 | 0.029
  (150,8,72,8,16)             (16,8,1) 16-byte         0.083 | 0.072   0.080 | 0.078
  (3,16,72,8,8)               (8,8,1) 16-byte          0.025 | 0.025   0.026 | 0.032
  (301,8,72,8,8)              (8,8,2) 16-byte          0.073 | 0.071   0.080 | 0.070
  (2,12,40,7,18)              (32,2,1) scalar          0.036 | 0.036   0.033 | 0.032
  (2,10,24,6,35)              (32,2,1) scalar          0.040 | 0.037   0.036 | 0.044
  (153,12,70,7,18)            (32,4,1) scalar          0.056 | 0.050   0.049 | 0.056
  (3,5,70,5,9)                (16,4,1) scalar          0.074 | 0.080   0.066 | 0.066
  (427,5,70,5,9)              (16,8,1) scalar          0.101 | 0.106   0.096 | 0.104
  (3,10,70,9,7)               (8,8,1) scalar           0.041 | 0.046   0.033 | 0.041
  (305,10,70,9,7)             (8,8,2) scalar           0.057 | 0.055   0.058 | 0.060
  (1200,8,64,4,8)             (8,8,1) 16-byte, big     0.073 | 0.070   0.073 | 0.073
  (2,3,40,6,16)               (16,4,1) CK = 4          0.123 | 0.127   0.090 | 0.086
  (2,4,70,5,33)               (32,2,1) CK = 4          0.095 | 0.101   0.128 | 0.108
  (2,8,24,13,13)              dense 13 x 13            0.045 | 0.045   0.054 | 0.045
  (the device's error is that of torch's float32 CPU convolution throughout: one chain in the same order)
  fused_pool_first_layer: pooled value 0.082 - 0.171 of the bound on the twelve rows, with and without bias; no window whose named position
      is below the fp64 maximum (0.000 of the two bounds); the c3 shape on the chunked kernel (y_pool or codes off 16 bytes) 0.119
  fused_pool_chunked_is_exact, unpooled_backward_data_is_exact, mixed_launch_equals_the_one_geometry_launch: bit for bit on every row;
      un-pooling backward-data against fp64 0.017 - 0.066 | 0.017 - 0.063
  weight_gradient_every_geometry: dw 0.000 - 0.003 of the bound on every row (float32 CPU 0.000 - 0.005: the bound grows with N H W, the
      error of a sum of mixed signs does not); db 0.005 - 0.542 units of 2^-24 sum|dy| (bound 3; the largest on (4,2,40,8,8) pooled);
      exactly splits slabs written on every row, on twice the workspace and on exactly clhip_conv3x3_bwd_weight_ws bytes
  unpooled_weight_gradient: bit for bit the dense gradient's on all 14 rows — conv3x3_wgrad_c3_unpool_kernel's two rows included,
      which the code does not promise and the test does not ask
  conv_operands_off_a_16_byte_boundary, weight_gradient_operands_off_a_16_byte_boundary: bit for bit the aligned result with every
      operand 1 and 2 floats off
  error_is_that_of_an_fp32_chain, all-positive operands, error / S in units of 2^-24 (max, rms): 3x3 kernel | clhip_conv2d_*
  (2,16,72,8,16) fwd             11.6  2.84 | 12.9  2.84      ratio 0.90 1.00
  (3,5,70,5,9) fwd               6.45  1.53 | 6.02  1.53      ratio 1.07 1.00
  (2,8,24,13,13) fwd             8.04  1.99 | 9.18  2.01      ratio 0.88 0.99
  (2,72,16,8,16) bwd_data        11.7  2.80 | 13.0  2.81      ratio 0.90 1.00
  (5,3,40,6,35) bwd_weight       1.54  0.59 | 6.89  2.07      ratio 0.22 0.29    (30 slabs summed in f64 against one float32 chain)
  (20,24,40,8,16) bwd_weight     1.10  0.44 | 5.06  1.25      ratio 0.22 0.35
  (1025,12,24,8,16) bwd_weight   1.84  0.61 | 1.79  0.63      ratio 1.03 0.98
  weight_gradient_three_by_three_tiles (234,136,136,8,8): dw 0.000 | 0.000 of the bound, db 0.020 units
  Run time on the MI355X: 171 tests in 10.6 s; 0.51 s for the largest (33,3,64,64,64) pooled case, at most 0.36 s for any other.

Mutation check, run once against scratch copies of the sources (one run of this file per mutant with CLHIP_LIB on the mutant library;
only load predicates, loop trip counts downwards, comparisons and launch counts change, so each stays in bounds; not part of the
repository).  Failing tests per mutant (168 in all):
  chunked kernel   16-byte staging `h < H - 1` (the last row reads 0)                 46: conv_every_geometry x26, unpooled_backward_data x11, ...
                   scalar staging `w > 0` (the first column reads 0)                  35: conv_every_geometry x20, conv_operands_off... x12, ...
                   n_chunks = Cin / CK (the tail chunk dropped)                       26: every Cin % CK row of conv_every_geometry x17, ...
                   mask `mk[r] >= 0.f`                                                40: the backward-data rows x23, unpooled_backward_data x11, ...
                   un-pooling `i0 <= c`                                               11: unpooled_backward_data_is_exact x11
                   pooled epilogue `>=` (last maximum)                                14: fused_pool_chunked_is_exact x14 (all rows)
                   mixed<32,4,2>: n_a one image short / mixed2: one unit short        5 / 10: the mixed rows of conv_every_geometry, fused_pool,
                                                                                      unpooled_backward_data and mixed_launch_equals...
  c3 kernel        halo `rok[1]` against H - 1 / last maximum                         6 / 6: fused_pool_first_layer, its six rows
  c3w64 kernel     halo row against H - 1 / last maximum                              6 / 6: fused_pool_first_layer, its six rows
  wgrad kernel     16-byte staging x row against H - 1                                19: weight_gradient_every_geometry x13, ..._off_a_16... x4, fp32_chain x2
                   scalar staging x column against W - 1                              10: weight_gradient_every_geometry x6, ..._off_a_16... x4
                   un-pooling `i0 <= c`                                               12: weight_gradient_every_geometry x6, unpooled_weight_gradient x6
                   st_end: `split + 1 < extra` (one block a stage short)              15: the rows with total_stages % splits != 0
  smallc kernel    halo row against H - 1 / un-pooling `a <= 1`                       11 / 12
  c3_unpool kernel `code <= want` / halo row `hrow + 2 >= H`                          2 / 2: its two rows of weight_gradient_every_geometry
  reduction        bwd_weight_impl sums splits + 1 slabs (inside every workspace)     42: weight_gradient_every_geometry x34 (every row: the sentinel
                                                                                      slab makes dw non-finite), ..._off_a_16... x5, fp32_chain x3
                   scalar loads `e + t + 1 < total` (a slab's last element dropped)   3 (of the 57 weight-gradient and reduction tests, run
                                                                                      alone): the two rows of weight_gradient_every_geometry
                                                                                      whose slab is no multiple of 4, reduce_of_one_slab_copies_it
No mutant survived.
"""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import conv3x3_dispatch as d
import conv_dispatch as cd
import conv_parity as cp
import torch_ref
from conv_parity import BYTE_OUT, OUT_BITS, U, WS_BITS, WS_SLACK, accuracy, check_ws, run_call, unit_errors
from kernel_parity import all_bits, bitwise_equal, ulp_distance

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC, ENOTSUP = -1, -2, -3


def full(s5):
    N, Cc, K, H, W = s5
    return (N, Cc, H, W, K, 3, 3, 1, 1)


def _sid(s5):
    return "x".join(str(v) for v in s5)


@functools.lru_cache(maxsize=None)
def seed_of(shape):
    for seed in range(8):
        try:
            cp.operands(shape, seed)
            return seed
        except AssertionError:
            pass
    raise AssertionError("no seed without a zero for %r" % (shape,))


@functools.lru_cache(maxsize=12)
def operands(s5, positive=False):
    return cp.operands(full(s5), seed_of(full(s5)), positive)


def codes_for(N, K, OH, OW):
    gen = torch.Generator().manual_seed(4242 + N * K + OH * OW)
    code = torch.randint(0, 5, (N, K, OH, OW), generator=gen, dtype=torch.uint8)
    for c in range(min(5, K)):
        code[0, c] = c
    code[N - 1, K - 1] = (torch.arange(OH * OW) % 5).to(torch.uint8).view(OH, OW)
    return code


@functools.lru_cache(maxsize=16)
def pooled_dy(s5):
    """(pooled gradient, codes, the dense dy torch_ref.unpool builds from them)."""
    N, Cc, K, H, W = s5
    gen = torch.Generator().manual_seed(99 + N * K * H * W)
    dyp = torch.randn((N, K, H // 2, W // 2), generator=gen)
    assert bool((dyp != 0).all())
    code = codes_for(N, K, H // 2, W // 2)
    return dyp, code, torch_ref.unpool(dyp, code)


@functools.lru_cache(maxsize=8)
def fwd_ref(s5, positive=False):
    x, w, _ = operands(s5, positive)
    return F.conv2d(x.double(), w.double(), None, 1, 1), F.conv2d(x, w, None, 1, 1), F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)


@functools.lru_cache(maxsize=8)
def bwd_ref(s5, pooled=False, positive=False):
    x, w, dy = operands(s5, positive)
    if pooled:
        dy = pooled_dy(s5)[2]
    return (conv2d_input(x.shape, w.double(), dy.double(), 1, 1), conv2d_input(x.shape, w, dy, 1, 1),
            conv2d_input(x.shape, w.double().abs(), dy.double().abs(), 1, 1))


@functools.lru_cache(maxsize=8)
def wg_ref(s5, pooled=False, positive=False):
    """(dw fp64, dw float32 CPU, S, db fp64, sum |dy|): the fp64 products as ONE GEMM over the unfolded input."""
    N, Cc, K, H, W = s5
    x, w, dy = operands(s5, positive)
    if pooled:
        dy = pooled_dy(s5)[2]
    xu = F.unfold(x.double(), 3, padding=1).permute(1, 0, 2).reshape(Cc * 9, N * H * W)
    dyf = dy.double().reshape(N, K, H * W).permute(1, 0, 2).reshape(K, N * H * W)
    dw64 = (dyf @ xu.t()).view(K, Cc, 3, 3)
    S = (dyf.abs() @ xu.abs().t()).view(K, Cc, 3, 3)
    return dw64, conv2d_weight(x, w.shape, dy, 1, 1), S, dyf.sum(1), dyf.abs().sum(1)


# --------------------------------------------------------------------------------------------- raw-pointer calls
def run_fwd(L, s5, x, w, bias=None, relu=0, mis=None, mis_by=1):
    N, Cc, K, H, W = s5

    def call(p, ws, nbytes, stream):
        return L.clhip_conv3x3_fwd(p["x"], p["w"], p["b"], p["out"], N, Cc, K, H, W, int(relu), stream)
    return run_call(call, [("x", x), ("w", w), ("b", bias)], [("out", N * K * H * W)], ws_floats=WS_SLACK, mis=mis, mis_by=mis_by)


def run_pool(L, s5, x, w, bias=None, mis=None, mis_by=1, idx_shift=0):
    N, Cc, K, H, W = s5
    n = N * K * (H // 2) * (W // 2)

    def call(p, ws, nbytes, stream):
        return L.clhip_conv3x3_relu_pool_fwd(p["x"], p["w"], p["b"], p["out"], p["idx"], N, Cc, K, H, W, stream)
    return run_call(call, [("x", x), ("w", w), ("b", bias)], [("out", n)], ws_floats=WS_SLACK, mis=mis, mis_by=mis_by, bouts=[("idx", n)],
                    bshift={"idx": idx_shift})


def run_bwd(L, s5, dy, w, src=None, code=None, mis=None, mis_by=1, idx_shift=2):
    """dy: the dense gradient, or with `code` the pooled one (clhip_conv3x3_bwd_data_unpool; codes at an even address by default)."""
    N, Cc, K, H, W = s5

    def call(p, ws, nbytes, stream):
        if code is not None:
            return L.clhip_conv3x3_bwd_data_unpool(p["dy"], p["idx"], p["w"], p["src"], p["out"], N, Cc, K, H, W, stream)
        return L.clhip_conv3x3_bwd_data(p["dy"], p["w"], p["src"], p["out"], N, Cc, K, H, W, stream)
    return run_call(call, [("dy", dy), ("w", w), ("src", src)], [("out", N * Cc * H * W)], ws_floats=WS_SLACK, mis=mis, mis_by=mis_by,
                    bins=[("idx", code)], bshift={"idx": idx_shift})


def run_wgrad(L, s5, x, dy, code=None, want_db=True, ws_bytes=None, exact=False, mis=None, mis_by=1, idx_shift=0, how="one"):
    """how: one = clhip_conv3x3_bwd_weight / _unpool; two = _slabs then _reduce.  exact: the arena's workspace ends WS_SLACK floats
    behind clhip_conv3x3_bwd_weight_ws bytes; otherwise it is twice that size and the call is told so."""
    N, Cc, K, H, W = s5
    need = d.ws_bytes(*s5) if ws_bytes is None else ws_bytes
    have = need if exact else 2 * need
    splits = []

    def call(p, ws, nbytes, stream):
        if how == "two":
            import ctypes as C
            so = C.c_int(-7)
            rc = L.clhip_conv3x3_bwd_weight_slabs(p["x"], p["dy"], p["idx"], N, Cc, K, H, W, ws, nbytes, C.byref(so), stream)
            splits.append(so.value)
            return rc if rc else L.clhip_conv3x3_bwd_weight_reduce(ws, p["out"], p["db"], K, Cc, so.value, stream)
        if code is not None:
            return L.clhip_conv3x3_bwd_weight_unpool(p["x"], p["dy"], p["idx"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
        return L.clhip_conv3x3_bwd_weight(p["x"], p["dy"], p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    r = run_call(call, [("x", x), ("dy", dy)], [("out", K * Cc * 9), ("db", K if want_db else None), ("nodb", None if want_db else K)],
                 ws_floats=have // 4 + WS_SLACK, ws_bytes=have, mis=mis, mis_by=mis_by, bins=[("idx", code)], bshift={"idx": idx_shift})
    r.splits = splits[0] if splits else None
    return r


def ok_call(r, what, touched=0):
    assert r.rc == 0 and r.clean, "%s: rc %d, gaps, guards or inputs changed: %s" % (what, r.rc, not r.clean)
    check_ws(r.ws, touched, what)


def written(t, what):
    assert not bool((t.view(torch.int32) == OUT_BITS).any()), "%s: an element was never written" % what


# --------------------------------------------------------------------------------------------- a. forward / backward-data
CONV = [(row, k) for row, _ in d.FWD_CASES for k in ("fwd", "bwd_data")]


def layer_of(kind, row):
    N, Cin, Cout, H, W = row
    return (N, Cin, Cout, H, W) if kind == "fwd" else (N, Cout, Cin, H, W)


def check_conv(case, L, kind, row, only=None, mis=None, mis_by=1):
    N, Cin, Cout, H, W = row
    s5 = layer_of(kind, row)
    Cc, K = s5[1], s5[2]
    x, w, dy = operands(s5)
    bias, src = cp.epilogue_inputs(full(s5))
    outs = {}
    if kind == "fwd":
        want, cpu, S = fwd_ref(s5)
        for name, kw, acc in (("bias-relu", dict(bias=bias, relu=1), dict(bias=bias, relu=True)), ("bias", dict(bias=bias), dict(bias=bias)), ("plain", {}, {})):
            if only is not None and name != only:
                continue
            r = run_fwd(L, s5, x, w, mis=mis, mis_by=mis_by, **kw)
            ok_call(r, name)
            accuracy(case, name, r.out["out"], want, cpu, S, 9 * Cc, 0, **acc)
            outs[name] = r.out["out"]
            assert all_bits(outs[name].view(N, K, H, W)[:, 0], 0), "%s: out-channel 0 must be exactly +0.0" % name
        if only is None:
            assert torch.equal(outs["bias-relu"], outs["bias"].clamp(min=0)), "relu is not max(v, 0) of the same v"
        return outs
    want, cpu, S = bwd_ref(s5)
    for name, kw, acc in (("relu_src", dict(src=src), dict(mask_src=src)), ("plain", {}, {})):
        if only is not None and name != only:
            continue
        r = run_bwd(L, s5, dy, w, mis=mis, mis_by=mis_by, **kw)
        ok_call(r, name)
        accuracy(case, name, r.out["out"], want, cpu, S, 9 * K, 0, **acc)
        outs[name] = r.out["out"]
    if only is None:
        on = src.reshape(-1) > 0
        assert bitwise_equal(outs["relu_src"][on], outs["plain"][on]), "relu_src > 0 must pass the value through unchanged"
        assert all_bits(outs["relu_src"][~on], 0), "relu_src of 0.0, -0.0, a negative denormal, NaN or a negative must give exactly +0.0"
    return outs


@pytest.mark.parametrize("row,kind", CONV, ids=["%s-%s" % (_sid(r), k) for r, k in CONV])
def test_conv_every_geometry(request, row, kind):
    """One row per arm of launch_conv, forward (no bias, bias, bias + ReLU) and backward-data (plain, relu_src).  The first assertion
    only ties the row to the restated rules (the arm, block counts and n_a that conv3x3_dispatch predicts for it); the library reports
    none of them, so the arm actually taken is not observed here — what is observed is the result of every element, and for the mixed
    rows the image-by-image equality of test_mixed_launch_equals_the_one_geometry_launch."""
    L = cp.product_lib()
    plan = dict(d.FWD_CASES)[row]
    s5 = layer_of(kind, row)
    got = d.fwd_plan(*s5) if kind == "fwd" else d.bwd_plan(*s5)
    assert (got.kernel, got.geo, got.blocks, got.n_a) == (plan.kernel, plan.geo, plan.blocks, plan.n_a)
    check_conv(request.node.name, L, kind, row)


# --------------------------------------------------------------------------------------------- b. fused pooling, chunked kernel
POOL_CHUNKED = [row for row, _ in d.FWD_CASES if not (row[3] | row[4]) & 1 and row[0] < 400] + [s for s, p in d.POOL_CASES if isinstance(p, d.FwdPlan)]


def window_view(t, N, K, H, W):
    return t.view(N, K, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, K, H // 2, W // 2, 4)


@pytest.mark.parametrize("row", POOL_CHUNKED, ids=[_sid(r) for r in POOL_CHUNKED])
def test_fused_pool_chunked_is_exact(row):
    """The pooled forward against clhip_conv3x3_fwd(relu = 1) of the same operands: value = the window maximum bit for bit, code = the first
    maximum in row-major order, 4 exactly where the value is 0.  Planted: out-channel 0 (four +0.0: code 4), out-channel 1 with zero
    weights and bias 0.25 (four equal positive values: code 0)."""
    L = cp.product_lib()
    N, Cc, K, H, W = row
    assert isinstance(d.pool_plan(*row), d.FwdPlan)
    x, w, _ = operands(row)
    bias, _ = cp.epilogue_inputs(full(row))
    w, bias = w.clone(), bias.clone()
    w[1] = 0.0
    bias[1] = 0.25
    dense = run_fwd(L, row, x, w, bias=bias, relu=1)
    ok_call(dense, "unpooled")
    r = run_pool(L, row, x, w, bias=bias, idx_shift=5)
    ok_call(r, "pooled")
    y, idx = r.out["out"].view(N, K, H // 2, W // 2), r.out["idx"].view(N, K, H // 2, W // 2)
    assert not bool((idx == BYTE_OUT).any()), "a window's code was never written"
    written(y, "pooled")
    win = window_view(dense.out["out"], N, K, H, W)
    m, a = win[..., 0].clone(), torch.zeros(idx.shape, dtype=torch.uint8)
    for i in (1, 2, 3):
        gt = win[..., i] > m
        m, a = torch.where(gt, win[..., i], m), torch.where(gt, torch.full_like(a, i), a)
    a = torch.where(m > 0, a, torch.full_like(a, 4))
    assert bitwise_equal(y, m), "the pooled value is not the maximum of the unpooled output's window"
    assert int((idx != a).sum()) == 0, "%d codes are not the first maximum in row-major order" % int((idx != a).sum())
    assert torch.equal(idx == 4, y == 0)
    assert bool((idx[:, 0] == 4).all()) and all_bits(y[:, 0], 0) and bool((idx[:, 1] == 0).all()) and bool((y[:, 1] == 0.25).all())


# --------------------------------------------------------------------------------------------- c. fused pooling, first-layer kernels
POOL_FIRST = [(s, p) for s, p in d.POOL_CASES if isinstance(p, d.PoolPlan)]


def check_first_layer_pool(case, r, s5, x, w, bias):
    N, Cc, K, H, W = s5
    y, idx = r.out["out"].view(N, K, H // 2, W // 2), r.out["idx"].view(N, K, H // 2, W // 2)
    assert not bool((idx == BYTE_OUT).any()) and int(idx.max()) <= 4, "a window's code was never written"
    written(y, "pooled")
    assert bool(torch.isfinite(y).all())
    bb = bias.double().view(1, -1, 1, 1)
    y64 = F.conv2d(x.double(), w.double(), None, 1, 1) + bb
    cpu = (F.conv2d(x, w, None, 1, 1) + bias.view(1, -1, 1, 1)).double()
    bound = (27 + 3) * U * F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1) + U * bb.abs()
    assert bool(((cpu - y64).abs() <= bound).all()), "torch's float32 CPU convolution misses the bound"
    yw, bw = window_view(y64, N, K, H, W), window_view(bound, N, K, H, W)
    live = idx < 4
    pos = idx.clamp(max=3).long().unsqueeze(-1)
    y_at, b_at = yw.gather(-1, pos).squeeze(-1), bw.gather(-1, pos).squeeze(-1)
    tiny = torch.finfo(torch.float64).tiny
    r_val = float((((y.double() - y_at.clamp(min=0)).abs() / b_at.clamp(min=tiny))[live]).max()) if bool(live.any()) else 0.0
    # the device's value at the named position p is >= its value at the fp64 arg-max q: y64[q] - y64[p] <= bound[p] + bound[q]
    q = yw.argmax(-1, keepdim=True)
    gap = (yw.gather(-1, q).squeeze(-1) - y_at) / (b_at + bw.gather(-1, q).squeeze(-1)).clamp(min=tiny)
    r_gap = float(gap[live].max()) if bool(live.any()) else 0.0
    dead = float(((yw - bw).amax(-1))[~live].max()) if bool((~live).any()) else -1.0      # a dead window: every y64 <= its bound
    print("MEASURED|%s|pooled value / bound|%.3f|-" % (case, r_val))
    print("MEASURED|%s|fp64 maximum above the named position / (two bounds)|%.3f|-" % (case, r_gap))
    assert r_val <= 1.0 and r_gap <= 1.0 and dead <= 0.0, (r_val, r_gap, dead)
    assert torch.equal(idx == 4, y == 0) and all_bits(y[idx == 4], 0), "code 4 exactly where the value is +0.0"


@pytest.mark.parametrize("s5,plan", POOL_FIRST, ids=[_sid(s) for s, _ in POOL_FIRST])
def test_fused_pool_first_layer(request, s5, plan):
    """conv3x3_c3w64_relu_pool_kernel / conv3x3_c3_relu_pool_kernel: per window the value against relu(fp64) at the position the code names,
    that position against the window's fp64 maximum, code 4 exactly at +0.0; the tie-break on planted channels: zero weights with bias
    -0.0 (channel 0: +0.0, code 4), +0.25 (channel 1: 0.25, code 0), -0.25 (channel 2: +0.0, code 4)."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    assert d.pool_plan(*s5) == plan
    x, w, _ = operands(s5)
    bias, _ = cp.epilogue_inputs(full(s5))
    w, bias = w.clone(), bias.clone()
    w[1], w[2] = 0.0, 0.0
    bias[1], bias[2] = 0.25, -0.25
    r = run_pool(L, s5, x, w, bias=bias)
    ok_call(r, "pooled")
    check_first_layer_pool(request.node.name, r, s5, x, w, bias)
    y, idx = r.out["out"].view(N, K, H // 2, W // 2), r.out["idx"].view(N, K, H // 2, W // 2)
    assert all_bits(y[:, 0], 0) and bool((idx[:, 0] == 4).all()), "channel 0"
    assert bool((y[:, 1] == 0.25).all()) and bool((idx[:, 1] == 0).all()), "channel 1: four equal positive values take code 0"
    assert all_bits(y[:, 2], 0) and bool((idx[:, 2] == 4).all()), "channel 2: a negative maximum is +0.0 with code 4"
    r0 = run_pool(L, s5, x, w, bias=None)                                   # no bias
    ok_call(r0, "pooled, no bias")
    check_first_layer_pool(request.node.name + "[no bias]", r0, s5, x, w, torch.zeros(K))
    r2 = run_pool(L, s5, x, w, bias=bias)
    assert bitwise_equal(r.out["out"], r2.out["out"]) and torch.equal(r.out["idx"], r2.out["idx"]), "two runs differ"


def test_first_layer_pool_off_a_16_byte_boundary():
    """x, w, bias one and two floats off on both first-layer kernels (they load dwords): the aligned bits.  y_pool or the codes off a 16-byte
    boundary: the c3w64 kernel stores dwords and bytes (same bits); the c3 kernel's shapes take the chunked kernel (within the rule)."""
    L = cp.product_lib()
    for s5 in ((3, 3, 70, 2, 64), (2, 3, 70, 10, 32)):
        N, Cc, K, H, W = s5
        x, w, _ = operands(s5)
        bias, _ = cp.epilogue_inputs(full(s5))
        base = run_pool(L, s5, x, w, bias=bias)
        ok_call(base, "aligned")
        for name, by, shift in (("x", 1, 0), ("x", 2, 0), ("w", 1, 0), ("w", 2, 0), ("b", 1, 0), ("out", 1, 0), ("out", 2, 0), (None, 1, 5), (None, 1, 2)):
            r = run_pool(L, s5, x, w, bias=bias, mis=name, mis_by=by, idx_shift=shift)
            ok_call(r, "%s + %d, codes + %d" % (name, by, shift))
            same_kernel = W == 64 or (name != "out" and shift == 0)
            assert d.pool_plan(*s5, out_aligned=(name != "out" and shift == 0)).kernel == ("c3w64" if W == 64 else ("c3" if same_kernel else "plain"))
            if same_kernel:
                assert bitwise_equal(r.out["out"], base.out["out"]) and torch.equal(r.out["idx"], base.out["idx"]), (s5, name, by, shift)
            else:
                check_first_layer_pool("c3 shape on the chunked kernel", r, s5, x, w, bias)


# --------------------------------------------------------------------------------------------- d. un-pooling
UNPOOL_BWD = [row for row, p in d.FWD_CASES if p.vec and not (row[3] | row[4]) & 1 and row[0] < 400]


@pytest.mark.parametrize("row", UNPOOL_BWD, ids=[_sid(r) for r in UNPOOL_BWD])
def test_unpooled_backward_data_is_exact(request, row):
    """clhip_conv3x3_bwd_data_unpool(pooled dy, codes) = clhip_conv3x3_bwd_data on the dense dy torch_ref.unpool builds, bit for bit, plain
    and behind relu_src; and within the rule of the fp64 result."""
    L = cp.product_lib()
    s5 = layer_of("bwd_data", row)
    N, Cc, K, H, W = s5
    assert d.bwd_plan(*s5, unpool=True) != ENOTSUP
    _, w, _ = operands(s5)
    _, src = cp.epilogue_inputs(full(s5))
    dyp, code, dense = pooled_dy(s5)
    assert set(code.reshape(-1).tolist()) == {0, 1, 2, 3, 4}
    want, cpu, S = bwd_ref(s5, pooled=True)
    for s in (None, src):
        a = run_bwd(L, s5, dyp, w, src=s, code=code)
        b = run_bwd(L, s5, dense, w, src=s)
        ok_call(a, "pooled")
        ok_call(b, "dense")
        accuracy(request.node.name, "pooled dy" + (" + relu_src" if s is not None else ""), a.out["out"], want, cpu, S, 9 * K, 0, mask_src=s)
        assert bitwise_equal(a.out["out"], b.out["out"]), "dx from pooled dy + codes differs from dx of the dense gradient"


# --------------------------------------------------------------------------------------------- e. weight gradient
WG_IDS = ["%s-%s-%s%s%s" % (_sid(c[0]), "pooled" if c[1] else "plain", c[3].name, "" if c[2][0] and c[2][1] else "-mis", "" if c[2][2] == 16 else "-idx%d" % c[2][2])
          for c in d.WG_CASES]
IDX_SHIFT = {16: 0, 2: 2, 1: 5}


def check_wgrad(case, L, wcase, exact=False, how="one", want_db=True, mis=None, mis_by=1):
    s5, pooled, al, kern, (splits, nbytes) = wcase
    N, Cc, K, H, W = s5
    x, _, dy = operands(s5)
    code = None
    if pooled:
        dy, code, _ = pooled_dy(s5)
    if mis is None:
        mis = "x" if not al[0] else ("dy" if not al[1] else None)
    dw64, dw32, S, db64, s_db = wg_ref(s5, pooled)
    r = run_wgrad(L, s5, x, dy, code=code, want_db=want_db, exact=exact, how=how, mis=mis, mis_by=mis_by, idx_shift=IDX_SHIFT[al[2]])
    ok_call(r, case, splits * (9 * K * Cc + K))
    if how == "two":
        assert r.splits == splits
    accuracy(case, "dw", r.out["out"], dw64, dw32, S, N * H * W, splits)
    if want_db:
        e = float(((r.out["db"].double() - db64).abs() / (U * s_db)).max())
        print("MEASURED|%s|db error in units of 2^-24 sum abs(dy), bound 3|%.3f|-" % (case, e))
        assert bool(torch.isfinite(r.out["db"]).all()) and e <= 3.0, "db: %.3f units" % e
        print("MEASURED|%s|db ulp from the rounded fp64 sum|%d|-" % (case, ulp_distance(r.out["db"], db64.float())))
    else:
        assert all_bits(r.out["nodb"], OUT_BITS), "db = NULL: the db-sized slot must keep its sentinel"
    return r


@pytest.mark.parametrize("wcase", d.WG_CASES, ids=WG_IDS)
def test_weight_gradient_every_geometry(request, wcase):
    """Every arm of bwd_weight_impl: exactly splits slabs written (on twice the workspace and on exactly clhip_conv3x3_bwd_weight_ws
    bytes), dw and db by the rules, _slabs + _reduce the same bits, a second call the same bits, db = NULL."""
    L = cp.product_lib()
    case = request.node.name
    s5, pooled, al, kern, (splits, nbytes) = wcase
    assert d.wg_kernel(*s5, pooled, *al) == kern and L.clhip_conv3x3_bwd_weight_ws(*s5) == nbytes
    r = check_wgrad(case, L, wcase)
    r2 = check_wgrad(case + "[exact ws]", L, wcase, exact=True)
    r3 = check_wgrad(case + "[slabs + reduce]", L, wcase, how="two")
    for other in (r2, r3):
        assert bitwise_equal(r.out["out"], other.out["out"]) and bitwise_equal(r.out["db"], other.out["db"]), "two calls differ"
    n = splits * (9 * s5[1] * s5[2] + s5[2])
    assert bitwise_equal(r.ws[:n], r3.ws[:n]), "the slabs of the two entry points differ"
    if s5[0] <= 400:
        r4 = check_wgrad(case + "[db=NULL]", L, wcase, want_db=False)
        assert bitwise_equal(r.out["out"], r4.out["out"]), "dw must not depend on db being asked for"


def test_weight_gradient_three_by_three_tiles(request):
    """The 64 x 64-tile kernel with 3 x 3 (k, c) tiles, the third of each 8 channels wide (K = C = 136): tile indexing beyond 2 x 2.  On
    exactly clhip_conv3x3_bwd_weight_ws bytes (22.7 MB), which keeps the row under the 40 MB of device tensors of this file."""
    L = cp.product_lib()
    wcase = d.TILES_3X3
    s5, pooled, al, kern, (splits, nbytes) = wcase
    assert d.wg_kernel(*s5, pooled, *al) == kern and L.clhip_conv3x3_bwd_weight_ws(*s5) == nbytes
    r = check_wgrad(request.node.name, L, wcase, exact=True)
    r2 = check_wgrad(request.node.name + "[slabs + reduce]", L, wcase, exact=True, how="two")
    assert bitwise_equal(r.out["out"], r2.out["out"]) and bitwise_equal(r.out["db"], r2.out["db"]), "two calls differ"


UNPOOL_WG = [c for c in d.WG_CASES if c[1]]


@pytest.mark.parametrize("wcase", UNPOOL_WG, ids=[i for i, c in zip(WG_IDS, d.WG_CASES) if c[1]])
def test_unpooled_weight_gradient(wcase):
    """dw, db from (pooled dy, codes) against dw, db from the dense dy: bit for bit on the general kernel and on the first-layer kernel
    with codes (the same kernel behind the LDS tile); conv3x3_wgrad_c3_unpool_kernel sums in another order: both within the rule
    (test_weight_gradient_every_geometry), the comparison printed."""
    L = cp.product_lib()
    s5, pooled, al, kern, _ = wcase
    x, _, _ = operands(s5)
    dyp, code, dense = pooled_dy(s5)
    mis = "x" if not al[0] else ("dy" if not al[1] else None)
    a = run_wgrad(L, s5, x, dyp, code=code, mis=mis, idx_shift=IDX_SHIFT[al[2]])
    b = run_wgrad(L, s5, x, dense, mis=mis)
    assert a.rc == 0 and a.clean and b.rc == 0 and b.clean
    same = bitwise_equal(a.out["out"], b.out["out"]) and bitwise_equal(a.out["db"], b.out["db"])
    print("MEASURED|%s|%s: bit for bit the dense gradient's|%d|-" % (_sid(s5), kern.name, same))
    if kern.name != "c3_unpool":
        assert same, "dw / db from pooled dy + codes differ from those of the dense gradient"


def test_reduce_of_one_slab_copies_it():
    """clhip_conv3x3_bwd_weight_reduce with splits = 1: dw[k][c][rs] = slab[rs][k][c] and db = the tail, bit for bit (float -> double -> float),
    splits = 3 of 4 slabs: the fourth is not read.  The slab holds K (9 C + 1) floats.  (5, 2): 95 and (5, 5): 230 are no multiples of 4 —
    wgrad_reduce_block's scalar loads, whose last thread is ragged (95 = 64 + 28 + 3, 230 = 3 * 64 + 36 + 2) and whose slabs 1, 2 start
    off a 16-byte boundary; (7, 3): 196 and (70, 9): 5740 are — its 16-byte loads.  With the slabs 1 and 2 floats off a 16-byte boundary
    the 16-byte loads may not be used either: the same bits, guards intact."""
    L = cp.product_lib()
    for K, Cc in ((5, 2), (5, 5), (7, 3), (70, 9)):
        slab = 9 * K * Cc + K
        assert (slab % 4 != 0) == (K == 5)
        gen = torch.Generator().manual_seed(K * Cc)
        part = torch.randn((4, slab), generator=gen)
        part[3] = float("nan")
        for splits in (1, 3):
            def call(p, ws, nbytes, stream):
                return L.clhip_conv3x3_bwd_weight_reduce(p["part"], p["out"], p["db"], K, Cc, splits, stream)
            want = part[0].double()
            for sp in range(1, splits):                        # the kernel's order: one slab per split-lane, the lanes added in order
                want = want + part[sp].double()
            dw = want[:9 * K * Cc].view(9, K * Cc).t().contiguous().view(-1)
            for mis, by in ((None, 1), ("part", 1), ("part", 2)):
                r = run_call(call, [("part", part)], [("out", 9 * K * Cc), ("db", K)], ws_floats=WS_SLACK, mis=mis, mis_by=by)
                ok_call(r, "reduce")
                written(r.out["out"], "dw")
                written(r.out["db"], "db")
                if splits == 1:
                    assert bitwise_equal(r.out["out"], dw.float()) and bitwise_equal(r.out["db"], want[9 * K * Cc:].float()), (K, Cc, mis, by)
                else:
                    assert torch.equal(r.out["out"], dw.float()) and torch.equal(r.out["db"], want[9 * K * Cc:].float()), "three slabs: the f64 sum rounded once"


# --------------------------------------------------------------------------------------------- f. refused calls write nothing
def untouched(r, rc, what):
    assert r.rc == rc, "%s: rc %d, expected %d" % (what, r.rc, rc)
    assert r.clean and all_bits(r.ws, WS_BITS), "%s: workspace or guards written" % what
    for k, v in r.out.items():
        assert all_bits(v, OUT_BITS) if v.dtype == torch.float32 else bool((v == BYTE_OUT).all()), "%s: %s written" % (what, k)


def test_refused_calls_write_nothing():
    L = cp.product_lib()
    x, w, dy = operands((2, 8, 16, 8, 8))
    s5 = (2, 8, 16, 8, 8)
    N, Cc, K, H, W = s5
    dyp, code, _ = pooled_dy(s5)
    # relu_pool_fwd on an odd map: EINVAL
    odd = (2, 8, 16, 7, 8)
    xo, wo, dyo = operands(odd)
    untouched(run_pool(L, odd, xo, wo), EINVAL, "relu_pool_fwd on an odd map")
    # bwd_data_unpool: odd map, a shape vec_ok refuses, codes at an odd address, dy off a 16-byte boundary
    untouched(run_bwd(L, odd, dyo[:, :, :3, :4].contiguous(), wo, code=torch.zeros((2, 16, 3, 4), dtype=torch.uint8)), ENOTSUP, "bwd_data_unpool on an odd map")
    s12 = (2, 8, 16, 8, 12)
    x12, w12, _ = operands(s12)
    untouched(run_bwd(L, s12, torch.ones((2, 16, 4, 6)), w12, code=torch.zeros((2, 16, 4, 6), dtype=torch.uint8)), ENOTSUP, "bwd_data_unpool, W % 16")
    untouched(run_bwd(L, s5, dyp, w, code=code, idx_shift=5), ENOTSUP, "bwd_data_unpool, odd code address")
    untouched(run_bwd(L, s5, dyp, w, code=code, mis="dy"), ENOTSUP, "bwd_data_unpool, dy off 16 bytes")
    # the weight gradient: a workspace one byte short (ENOSPC), codes on an odd map, codes off the 16-byte staging (ENOTSUP)
    need = d.ws_bytes(*s5)
    for how in ("one", "two"):
        r = run_wgrad(L, s5, x, dy, ws_bytes=need - 1, exact=True, how=how)    # one byte short
        untouched(r, ENOSPC, "weight gradient on a workspace one byte short (%s)" % how)
        assert run_wgrad(L, s5, x, dy, ws_bytes=need, exact=True, how=how).rc == 0, "exactly clhip_conv3x3_bwd_weight_ws bytes are enough"
        untouched(run_wgrad(L, odd, xo, torch.ones((2, 16, 3, 4)), code=torch.zeros((2, 16, 3, 4), dtype=torch.uint8), how=how), ENOTSUP, "codes on an odd map")
        untouched(run_wgrad(L, s5, x, dyp, code=code, idx_shift=5, how=how), ENOTSUP, "general kernel, odd code address")
        untouched(run_wgrad(L, s5, x, dyp, code=code, mis="x", how=how), ENOTSUP, "general kernel with codes, x off 16 bytes")
    # bwd_weight_unpool without codes, _slabs without splits_out, _reduce with splits <= 0: EINVAL, on real operands and a full workspace
    wsf = need // 4 + WS_SLACK

    def wg_u_no_codes(p, ws, nbytes, stream):
        return L.clhip_conv3x3_bwd_weight_unpool(p["x"], p["dy"], None, p["out"], p["db"], N, Cc, K, H, W, ws, nbytes, stream)
    untouched(run_call(wg_u_no_codes, [("x", x), ("dy", dyp)], [("out", 9 * K * Cc), ("db", K)], ws_floats=wsf, ws_bytes=need), EINVAL,
              "bwd_weight_unpool without codes")

    def slabs_no_splits_out(p, ws, nbytes, stream):
        return L.clhip_conv3x3_bwd_weight_slabs(p["x"], p["dy"], None, N, Cc, K, H, W, ws, nbytes, None, stream)
    untouched(run_call(slabs_no_splits_out, [("x", x), ("dy", dy)], [], ws_floats=wsf, ws_bytes=need), EINVAL, "_slabs without splits_out")
    part = torch.randn((2, 9 * K * Cc + K), generator=torch.Generator().manual_seed(5))
    for bad in (0, -1):
        def reduce_bad(p, ws, nbytes, stream):
            return L.clhip_conv3x3_bwd_weight_reduce(p["part"], p["out"], p["db"], K, Cc, bad, stream)
        untouched(run_call(reduce_bad, [("part", part)], [("out", 9 * K * Cc), ("db", K)], ws_floats=WS_SLACK), EINVAL, "_reduce with splits = %d" % bad)
    # the bf16-split entry points with codes on an odd map: refused ahead of the weight launch
    b5 = (2, 64, 64, 5, 9)
    xb, wb, dyb = operands(b5)
    need = L.clhip_conv3x3_bs_ws(64, 64)

    def bs_fwd(p, ws, nbytes, stream):
        return L.clhip_conv3x3_bs_fwd(p["x"], p["w"], None, p["out"], p["idx"], 2, 64, 64, 5, 9, 1, ws, nbytes, stream)
    untouched(run_call(bs_fwd, [("x", xb), ("w", wb)], [("out", 2 * 64 * 45)], ws_floats=need // 4 + WS_SLACK, ws_bytes=need, bouts=[("idx", 2 * 64 * 8)]),
              ENOTSUP, "clhip_conv3x3_bs_fwd with codes on an odd map")

    def bs_bwd(p, ws, nbytes, stream):
        return L.clhip_conv3x3_bs_bwd_data(p["dy"], p["idx"], p["w"], None, p["out"], 2, 64, 64, 5, 9, ws, nbytes, stream)
    untouched(run_call(bs_bwd, [("dy", torch.ones(2 * 64 * 8)), ("w", wb)], [("out", 2 * 64 * 45)], ws_floats=need // 4 + WS_SLACK, ws_bytes=need,
                       bins=[("idx", torch.zeros(2 * 64 * 8, dtype=torch.uint8))]), ENOTSUP, "clhip_conv3x3_bs_bwd_data with codes on an odd map")


# --------------------------------------------------------------------------------------------- g. off a 16-byte boundary
MIS_ROWS = [(2, 16, 72, 4, 32), (2, 16, 72, 8, 16), (3, 16, 72, 8, 8), (3, 5, 70, 5, 9), (2, 8, 24, 13, 13), (2, 3, 40, 6, 16)]
MIS = [(row, k) for row in MIS_ROWS for k in ("fwd", "bwd_data")]


@pytest.mark.parametrize("row,kind", MIS, ids=["%s-%s" % (_sid(r), k) for r, k in MIS])
def test_conv_operands_off_a_16_byte_boundary(request, row, kind):
    """x, w, bias, y (dy, w, relu_src, dx) in turn one and two floats past a 16-byte boundary: x | w (dy | w) off selects the scalar-staging
    instantiation, which fills the same LDS planes: clean, within the rule, the aligned result's bits."""
    L = cp.product_lib()
    s5 = layer_of(kind, row)
    aligned_vec = d.fwd_vec(s5[1], *s5[3:]) if kind == "fwd" else d.bwd_vec(*s5[1:])
    assert not (d.fwd_vec(s5[1], *s5[3:], aligned=False) if kind == "fwd" else d.bwd_vec(*s5[1:], aligned=False))
    variant = "bias-relu" if kind == "fwd" else "relu_src"
    base = check_conv(request.node.name, L, kind, row, only=variant)[variant]
    for name in (("x", "w", "b", "out") if kind == "fwd" else ("dy", "w", "src", "out")):
        for by in (1, 2):
            got = check_conv("%s[%s+%d]" % (request.node.name, name, by), L, kind, row, only=variant, mis=name, mis_by=by)[variant]
            assert bitwise_equal(got, base), "%s %d floats off (16-byte staging when aligned: %s): the result changed" % (name, by, aligned_vec)


MIS_WG = [c for c in d.WG_CASES if not c[1] and c[2] == d.AL and c[0] in ((5, 3, 40, 6, 35), (20, 24, 40, 8, 16), (10, 24, 40, 4, 32), (100, 64, 64, 8, 8), (1025, 12, 24, 8, 16))]


@pytest.mark.parametrize("wcase", MIS_WG, ids=[_sid(c[0]) for c in MIS_WG])
def test_weight_gradient_operands_off_a_16_byte_boundary(request, wcase):
    """x, dy, dw, db in turn one and two floats off: x | dy off selects the scalar staging of the same kernel, which fills the same LDS
    tiles: the aligned result's bits."""
    L = cp.product_lib()
    assert len(MIS_WG) == 5
    base = check_wgrad(request.node.name, L, wcase)
    for name in ("x", "dy", "out", "db"):
        for by in (1, 2):
            r = check_wgrad("%s[%s+%d]" % (request.node.name, name, by), L, wcase, mis=name, mis_by=by)
            assert bitwise_equal(r.out["out"], base.out["out"]) and bitwise_equal(r.out["db"], base.out["db"]), "%s %d floats off: the result changed" % (name, by)


# --------------------------------------------------------------------------------------------- h. mixed launches
MIXED = [(row, plan) for row, plan in d.FWD_CASES if plan.kernel.startswith("mixed")]


@pytest.mark.parametrize("row,plan", MIXED, ids=[_sid(r) for r, _ in MIXED])
def test_mixed_launch_equals_the_one_geometry_launch(row, plan):
    """Forward, pooled forward, backward-data and un-pooling backward-data of a mixed-launch row: the first images, the images around
    n_a and the last images equal, bit for bit, the same entry point on a batch of two (one geometry, not `big`)."""
    L = cp.product_lib()
    N, Cin, Cout, H, W = row
    n_a = plan.n_a
    pairs = [0, n_a - 2, n_a - 1, n_a, N - 2]
    fl, bl = (N, Cin, Cout, H, W), (N, Cout, Cin, H, W)
    assert d.pool_plan(*fl).n_a == n_a and d.bwd_plan(*bl).n_a == n_a and d.bwd_plan(*bl, unpool=True).n_a == n_a
    x, w, _ = operands(fl)
    bias, _ = cp.epilogue_inputs(full(fl))
    _, wb, dy = operands(bl)
    _, src = cp.epilogue_inputs(full(bl))
    dyp, code, _ = pooled_dy(bl)
    big = dict(fwd=run_fwd(L, fl, x, w, bias=bias, relu=1), pool=run_pool(L, fl, x, w, bias=bias, idx_shift=5), bwd=run_bwd(L, bl, dy, wb, src=src),
               unpool=run_bwd(L, bl, dyp, wb, src=src, code=code))
    for r in big.values():
        ok_call(r, "mixed launch")
    for i in pairs:
        f2, b2 = (2,) + fl[1:], (2,) + bl[1:]
        assert d.fwd_plan(*f2).kernel == "plain" and d.bwd_plan(*b2).kernel == "plain"
        small = dict(fwd=run_fwd(L, f2, x[i:i + 2], w, bias=bias, relu=1), pool=run_pool(L, f2, x[i:i + 2], w, bias=bias, idx_shift=5),
                     bwd=run_bwd(L, b2, dy[i:i + 2], wb, src=src[i:i + 2]), unpool=run_bwd(L, b2, dyp[i:i + 2], wb, src=src[i:i + 2], code=code[i:i + 2]))
        for k, r in small.items():
            ok_call(r, k)
            for name, t in r.out.items():
                per = t.numel() // 2
                assert bitwise_equal(big[k].out[name][i * per:(i + 2) * per], t) if t.dtype == torch.float32 else torch.equal(big[k].out[name][i * per:(i + 2) * per], t), \
                    "%s: images %d, %d of the mixed launch differ from the batch of two" % (k, i, i + 1)


# --------------------------------------------------------------------------------------------- i. locality of NaN and Inf
LOCAL = [(2, 16, 72, 4, 32), (2, 16, 72, 8, 16), (3, 16, 72, 8, 8), (3, 5, 70, 5, 9), (2, 12, 40, 7, 18), (2, 8, 24, 13, 13), (2, 3, 40, 6, 16)]


@pytest.mark.parametrize("row", LOCAL, ids=[_sid(r) for r in LOCAL])
def test_nan_and_inf_stay_in_their_support(row):
    """One NaN (interior) and one Inf (a tile corner: the last row and column of the first tile, or of the map) planted in x / dy: exactly the
    outputs of that image whose 3 x 3 window holds them are non-finite, in every out-channel."""
    L = cp.product_lib()
    for kind in ("fwd", "bwd_data"):
        s5 = layer_of(kind, row)
        N, Cc, K, H, W = s5
        x, w, dy = operands(s5)
        t = (x if kind == "fwd" else dy).clone()
        w = w.clone()
        w[0] = 0.05                                        # no zero channel: 0 * Inf would be NaN all the same, but keep every channel a real sum
        geo = dict(d.FWD_CASES).get(row)
        tw, th = (geo.geo[0], geo.geo[1]) if geo else (16, 4)
        spots = [(0, 1, min(2, H - 1), min(3, W - 1), float("nan")), (N - 1, t.shape[1] - 1, min(th, H) - 1, min(tw, W) - 1, float("inf"))]
        want = torch.zeros((N, H, W), dtype=torch.bool)
        for n, c, h, ww, v in spots:
            t[n, c, h, ww] = v
            want[n, max(h - 1, 0):h + 2, max(ww - 1, 0):ww + 2] = True
        r = run_fwd(L, s5, t, w) if kind == "fwd" else run_bwd(L, s5, t, w)
        assert r.rc == 0 and r.clean
        out = r.out["out"].view(N, -1, H, W)
        bad = ~torch.isfinite(out)
        assert torch.equal(bad, want.unsqueeze(1).expand_as(bad)), "%s: %d non-finite outputs, %d expected" % (kind, int(bad.sum()), int(want.sum()) * out.shape[1])


# --------------------------------------------------------------------------------------------- quality of the rounding
COHERENT = [("fwd", (2, 16, 72, 8, 16)), ("fwd", (3, 5, 70, 5, 9)), ("fwd", (2, 8, 24, 13, 13)), ("bwd_data", (2, 72, 16, 8, 16)),
            ("bwd_weight", (5, 3, 40, 6, 35)), ("bwd_weight", (20, 24, 40, 8, 16)), ("bwd_weight", (1025, 12, 24, 8, 16))]


@pytest.mark.parametrize("kind,s5", COHERENT, ids=["%s-%s" % (_sid(s), k) for k, s in COHERENT])
def test_error_is_that_of_an_fp32_chain(request, kind, s5):
    """All-positive operands: rounding errors add up instead of cancelling.  error / S in units of 2^-24 (max, rms) next to clhip_conv2d_* on
    the same layer: measurements (the table in the header); asserted is the rule alone."""
    L = cp.product_lib()
    N, Cc, K, H, W = s5
    shape = full(s5)
    x, w, dy = operands(s5, positive=True)
    if kind == "fwd":
        want, cpu, S = fwd_ref(s5, positive=True)
        r = run_fwd(L, s5, x, w)
        ins, outs, Kd, splits = [("x", x), ("w", w)], [("out", N * K * H * W)], 9 * Cc, 0

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_fwd(p["x"], p["w"], None, p["out"], *shape, 0, stream)
    elif kind == "bwd_data":
        want, cpu, S = bwd_ref(s5, positive=True)
        r = run_bwd(L, s5, dy, w)
        ins, outs, Kd, splits = [("dy", dy), ("w", w)], [("out", N * Cc * H * W)], 9 * K, 0

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_data(p["dy"], p["w"], None, p["out"], *shape, stream)
    else:
        want, cpu, S = wg_ref(s5, positive=True)[:3]
        r = run_wgrad(L, s5, x, dy)
        ins, outs, Kd, splits = [("x", x), ("dy", dy)], [("out", K * Cc * 9)], N * H * W, d.make_plan(*s5).splits

        def call(p, ws, nbytes, stream):
            return L.clhip_conv2d_bwd_weight(p["x"], p["dy"], p["out"], None, *shape, ws, nbytes, stream)
    assert r.rc == 0 and r.clean
    accuracy(request.node.name, "positive operands", r.out["out"], want, cpu, S, Kd, splits)
    f = run_call(call, ins, outs, ws_floats=cd.bwd_weight_ws_bytes(shape) // 4)
    assert f.rc == 0 and f.clean
    a, b = unit_errors(r.out["out"], want, S), unit_errors(f.out["out"], want, S)
    print("MEASURED|%s|error / S (max, rms) in units of 2^-24: 3x3 kernel %.3f %.3f, clhip_conv2d %.3f %.3f|%.3f|%.3f"
          % (request.node.name, a[0] / U, a[1] / U, b[0] / U, b[1] / U, a[0] / max(b[0], 1e-300), a[1] / max(b[1], 1e-300)))
