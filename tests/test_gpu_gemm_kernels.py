"""Kernel-level parity of csrc/gemm.hip + csrc/gemm_body.hpp: clhip_fc_fwd, clhip_fc_bwd_data and clhip_fc_bwd_weight called
with raw pointers into one kernel_parity.Arena (operands, outputs and the workspace between sentinel gaps), each against the
fp64 product of the same float32 inputs.

Dispatch.  gemm_dispatch.py restates wide_ok, choose_splits, choose_splits_wide, k_per_split, the live split count and the
workspace one call needs; gemm_dispatch.CASES says for every (M, I, O) and entry point which tile kernel runs and how many
splits it launches, and every case asserts that the restated rules reproduce its row.  What a test can OBSERVE of that is the
workspace: it starts as a NaN with a fixed payload and is compared bit for bit afterwards — with more than one split predicted
exactly the first M*N*splits floats have changed and nothing behind them, with one split nothing has.  Wide versus 64x64
cannot be observed this way when the two split rules give the same count (every single-split wide case, and backward-data
(132,1028,260) / backward-weight (260,1024,128) where both give 2); for those the statement that tells the two kernels
apart is test_wide_tile_equals_64_tile_bitwise, which runs the same pointers through a library built with
CLHIP_NO_WIDE_GEMM.  A declined wide kernel IS visible for forward (129,324,1025): 2 splits wide, 3 splits on 64x64 tiles.

Accuracy rule, per element (not per tensor): |device - fp64| <= (K + splits + 3) * 2^-24 * (|A| . |B|)[m][n] + 2^-24 * |bias[n]|,
the forward error bound of a K-term float32 dot product in any summation order (gamma_K), the split-K adds and the bias add;
ReLU and the mask are 1-Lipschitz or exact and do not enlarge it.  torch's float32 CPU matmul has to satisfy the same bound
(a sanity condition on the inputs).  db (colsum_kernel, double accumulator, one rounding) is within 1 ulp of the float32
rounding of the fp64 column sum.

Measured on one MI355X (worst element of a case over its epilogue variants: device error / bound, float32-CPU error / bound;
every check prints `MEASURED|case|what|device/bound|float32 CPU/bound` before it asserts, run with -s):
  fc_every_path (M, I, O)      fwd             bwd_data        bwd_weight
  (1,1,1)                     0.033 / 0.033   0.003 / 0.003   0.038 / 0.038
  (7,50,33)                   0.057 / 0.030   0.057 / 0.057   0.220 / 0.223
  (33,97,31)                  0.032 / 0.032   0.095 / 0.071   0.079 / 0.079
  (65,500,65)                 0.005 / 0.003   0.057 / 0.057   0.055 / 0.055
  (3,500,5)                   0.001 / 0.001   0.205 / 0.250   0.251 / 0.317
  (5,3000,7)                  0.001 / 0.000   0.271 / 0.271   0.305 / 0.305
  (64,3104,64)                0.001 / 0.000   0.064 / 0.064   0.082 / 0.082
  (200,128,20)                0.021 / 0.021   0.153 / 0.153   0.011 / 0.008
  (130,36,1027)               0.112 / 0.112   0.002 / 0.003   0.036 / 0.036
  (129,324,1025)              0.014 / 0.007   0.003 / 0.003   0.040 / 0.040
  (132,388,1028)              0.010 / 0.007   0.003 / 0.001   0.042 / 0.042
  (130,1028,132)              0.005 / 0.001   0.036 / 0.036   0.033 / 0.033
  (132,1028,260)              0.004 / 0.001   0.018 / 0.011   0.033 / 0.033
  (260,1024,128)              0.004 / 0.001   0.043 / 0.043   0.018 / 0.009
  (128,1024,4)                0.002 / 0.001   0.387 / 0.387   0.025 / 0.025
  wide_kernel_declines
    130x36x1027-fwd-Amisaligned                         0.112 / 0.112
    130x36x1027-fwd-Bmisaligned                         0.112 / 0.112
    129x324x1025-fwd-Amisaligned                        0.007 / 0.007
    129x324x1025-fwd-Bmisaligned                        0.007 / 0.007
    130x38x1027-fwd-Kmod4                               0.093 / 0.093
    130x1028x132-bwd_data-Amisaligned                   0.030 / 0.030
    130x1028x132-bwd_data-Bmisaligned                   0.030 / 0.030
    132x1028x260-bwd_data-Amisaligned                   0.009 / 0.010
    132x1028x260-bwd_data-Bmisaligned                   0.009 / 0.010
    130x1028x38-bwd_data-Kmod4                          0.097 / 0.097
    130x1026x132-bwd_data-Nmod4                         0.024 / 0.024
    132x1028x260-bwd_weight-Amisaligned                 0.033 / 0.033
    132x1028x260-bwd_weight-Bmisaligned                 0.033 / 0.033
    260x1024x128-bwd_weight-Amisaligned                 0.011 / 0.009
    260x1024x128-bwd_weight-Bmisaligned                 0.011 / 0.009
    38x1028x260-bwd_weight-Kmod4                        0.152 / 0.152
    132x1028x258-bwd_weight-Mmod4                       0.032 / 0.032
    132x1026x260-bwd_weight-Nmod4                       0.035 / 0.035
  wide_tile_equals_64_tile_bitwise (worse of the two libraries)
    130x36x1027-fwd                                     0.112 / 0.112
    129x324x1025-fwd                                    0.008 / 0.007
    132x388x1028-fwd                                    0.006 / 0.007
    130x1028x132-bwd_data                               0.036 / 0.036
    132x1028x260-bwd_data                               0.010 / 0.011
    132x1028x260-bwd_weight                             0.033 / 0.033
    260x1024x128-bwd_data                               0.043 / 0.043
    260x1024x128-bwd_weight                             0.011 / 0.009
    128x1024x4-bwd_data                                 0.387 / 0.387
  db: 0 ulp from the rounded fp64 column sum in every case that asks for it (colsum_rounds_once and all of the above)
  Run time on the MI355X: 83 tests in 3.0 s; 0.29 s for the first (library load), at most 0.07 s for any other.

Mutation check, run once against scratch copies of the two sources (each mutant stays in bounds; one run of this file per
mutant with CLHIP_LIB on the mutant library; not part of the repository):
  (a) an empty split returns before its store          13 fail: fc_every_path x11 (every case with an empty split: "a slab element
                                                       of the ... promised floats was not written"), non_finite_stays... x2
  (b) `k < k_end` -> `k < K` in the 64-tile loads      none fails, and none can: EQUIVALENT.  k_per_split is a multiple of the
  (c) the same in the wide kernel's loads              32-deep chunk, so a chunk of a split that is not the last live one never
                                                       reaches k_end, and for the last live one k_end == K; the loops still stop
                                                       at k_end.  The two conditions select the same elements in every launch.
  (b2) (b) plus the chunk loop running to K            18 fail: fc_every_path x12, wide_kernel_declines x6 (accuracy rule, thousands of times the bound)
  (c2) (c) plus the chunk loop running to K            8 fail: fc_every_path x4, wide_tile_equals... x4 (every wide case with more than one split)
  (d) the reduce kernel reads bias[e % M]              12 fail: fc_every_path x8, wide_kernel_declines x2, wide_tile_equals... x2
                                                       (accuracy rule, 10x to 4000x the bound; M == N in (65,500,65) and (64,3104,64))
  (e) the mask uses `>= 0`                             25 fail: every backward-data case of fc_every_path x15, declines x6,
                                                       wide_tile_equals... x4 (a 0.0 / -0.0 mask entry lets the value through)
  (f) colsum_kernel: per = M / 16                      24 fail: colsum_rounds_once x4 (all but M = 16), every backward-weight case
                                                       of fc_every_path whose batch is no multiple of 16 x13, declines x7
  (g) fallback compares ws_bytes with mn, not          16 fail: every split case of fc_every_path, at "(b) ws_bytes = need - 1:
      mn * splits                                      workspace written"
  (h) wide_ok ignores aligned16                        not built: whether a 16-byte global load from an address that is only
                                                       4-byte aligned is harmless on gfx950 cannot be settled by reading this
                                                       code, and a mutant that may fault is not run
"""
import ctypes as C
import functools
import os

import pytest
import torch

import gemm_dispatch as gd
from kernel_parity import Arena, all_bits, bitwise_equal, ulp_distance

pytestmark = pytest.mark.gpu

WS_BITS = 0x7FC0BEEF          # workspace before a call: a quiet NaN, payload 0xBEEF
OUT_BITS = 0x7FC00A11         # outputs before a call: another NaN, so an element that was never written is not finite
WS_SLACK = 64                 # floats of workspace handed over beyond what a call needs
U = 2.0 ** -24                # unit roundoff of float32
ENTRY = {"fwd": "clhip_fc_fwd", "bwd_data": "clhip_fc_bwd_data", "bwd_weight": "clhip_fc_bwd_weight"}


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def product_lib():
    from clsurvey_amd import _lib
    return _lib.lib()


# --------------------------------------------------------------------------------------------- problems and references
def operands(kind, shape, seed=0):
    """Host operands of one entry point as (first, second) in GEMM order — A then B — and their logical views A[M][K], B[K][N]
    (views share storage, so writing through a view changes the operand).  Activations ~ N(0,1), weights ~ 0.05 N(0,1)."""
    M, I, O = shape
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * I + O + gd.KINDS.index(kind))
    if kind == "fwd":
        x, w = torch.randn((M, I), generator=gen), torch.randn((O, I), generator=gen) * 0.05
        return x, w, x, w.t()
    if kind == "bwd_data":
        dy, w = torch.randn((M, O), generator=gen), torch.randn((O, I), generator=gen) * 0.05
        return dy, w, dy, w
    dy, x = torch.randn((M, O), generator=gen), torch.randn((M, I), generator=gen)
    return dy, x, dy.t(), x


def epilogue_inputs(kind, shape):
    """bias[N] for forward; relu_src[M][N] for backward-data with exact 0.0, -0.0 and negative entries planted."""
    g = gd.fc_gemm(kind, *shape)
    gen = torch.Generator().manual_seed(77 + g.M + g.N)
    bias = torch.randn((g.N,), generator=gen) * 0.1
    src = torch.randn((g.M * g.N,), generator=gen)
    src[0::5] = 0.0
    src[1::5] = -0.0
    src[2::5] = -src[2::5].abs() - 1e-30
    return bias, src.view(g.M, g.N)


class Ref:
    def __init__(self, Av, Bv):
        self.c64 = Av.double() @ Bv.double()
        self.absab = Av.double().abs() @ Bv.double().abs()
        self.c32 = Av @ Bv                                    # torch's own float32 CPU product


@functools.lru_cache(maxsize=None)
def reference(kind, shape):
    a, b, Av, Bv = operands(kind, shape)
    return Ref(Av, Bv)


def accuracy(case, what, got, ref, K, splits, bias=None, relu=False, mask_src=None):
    """The per-element rule of the module docstring; returns the worst device and float32-CPU ratios to the bound."""
    bound = (K + splits + 3) * U * ref.absab
    want, cpu = ref.c64, ref.c32
    if bias is not None:
        bound = bound + U * bias.double().abs()
        want, cpu = want + bias.double(), cpu + bias
    if relu:
        want, cpu = want.clamp(min=0), cpu.clamp(min=0)
    if mask_src is not None:
        want, cpu = want * (mask_src > 0), cpu * (mask_src > 0)
    got = got.view(want.shape)
    finite = bool(torch.isfinite(got).all())
    tiny = torch.finfo(torch.float64).tiny
    r_dev = float(((got.double() - want).abs() / bound.clamp(min=tiny)).max()) if finite else float("inf")
    r_cpu = float(((cpu.double() - want).abs() / bound.clamp(min=tiny)).max())
    print("MEASURED|%s|%s|%.3f|%.3f" % (case, what, r_dev, r_cpu))
    assert r_cpu <= 1.0, "%s: torch's float32 CPU product misses the bound (%.3f of it): the inputs do not suit the rule" % (what, r_cpu)
    assert finite, "%s: non-finite output (an element never written, or stale workspace summed)" % what
    assert r_dev <= 1.0, "%s: %.3f of the derived bound (K = %d, splits = %d)" % (what, r_dev, K, splits)
    return r_dev, r_cpu


# --------------------------------------------------------------------------------------------- one call
class Run:
    pass


def run_fc(L, kind, shape, a, b, bias=None, relu=0, relu_src=None, want_db=False, ws_floats=0, ws_bytes=None, ws_null=False,
           mis_a=False, mis_b=False):
    """One call of an entry point on a fresh arena.  ws_floats: size of the workspace slot; ws_bytes: what the call is told
    (default: all of it); ws_null: the slot exists but NULL is passed."""
    M, I, O = shape
    g = gd.fc_gemm(kind, M, I, O)
    ar = Arena()
    ka, kb = ar.add(a, misaligned=mis_a), ar.add(b, misaligned=mis_b)
    kbias = ar.add(bias) if bias is not None else None
    ksrc = ar.add(relu_src) if relu_src is not None else None
    kout = ar.add(g.M * g.N, fill=OUT_BITS)
    kdb = ar.add(O, fill=OUT_BITS) if kind == "bwd_weight" else None
    kws = ar.add(max(ws_floats, 4), fill=WS_BITS)
    ar.upload(dev())
    assert ar.ptr(ka) % 16 == (4 if mis_a else 0) and ar.ptr(kb) % 16 == (4 if mis_b else 0)
    ws = None if ws_null else ar.ptr(kws)
    nbytes = 4 * ws_floats if ws_bytes is None else ws_bytes
    stream = torch.cuda.current_stream().cuda_stream
    if kind == "fwd":
        rc = L.clhip_fc_fwd(ar.ptr(ka), ar.ptr(kb), ar.ptr(kbias) if bias is not None else None, ar.ptr(kout), M, I, O, int(relu),
                            ws, nbytes, stream)
    elif kind == "bwd_data":
        rc = L.clhip_fc_bwd_data(ar.ptr(ka), ar.ptr(kb), ar.ptr(ksrc) if relu_src is not None else None, ar.ptr(kout), M, I, O,
                                 ws, nbytes, stream)
    else:                                              # (x, dy, dw, db): the GEMM's A is dy, its B is x
        rc = L.clhip_fc_bwd_weight(ar.ptr(kb), ar.ptr(ka), ar.ptr(kout), ar.ptr(kdb) if want_db else None, M, I, O, ws, nbytes, stream)
    torch.cuda.synchronize()
    ar.download()
    r = Run()
    r.rc, r.out, r.ws = rc, ar.get(kout).clone(), ar.get(kws).clone()
    r.db = ar.get(kdb).clone() if kdb is not None else None
    r.clean = ar.gaps_untouched() and bitwise_equal(ar.get(ka), a.reshape(-1)) and bitwise_equal(ar.get(kb), b.reshape(-1)) \
        and (bias is None or bitwise_equal(ar.get(kbias), bias)) and (relu_src is None or bitwise_equal(ar.get(ksrc), relu_src.reshape(-1)))
    return r


def check_ws(r, touched, what):
    """Exactly the first `touched` floats of the workspace changed (every slab element is written, and with a finite value),
    nothing behind them did."""
    head, rest = r.ws[:touched], r.ws[touched:]
    assert all_bits(rest, WS_BITS), "%s: workspace written behind its first %d floats" % (what, touched)
    if touched:
        assert bool(torch.isfinite(head).all()), "%s: a slab element of the %d promised floats was not written" % (what, touched)


def variants(kind, shape):
    """Epilogue variants of an entry point: (name, kwargs for run_fc, kwargs for accuracy)."""
    bias, src = epilogue_inputs(kind, shape)
    if kind == "fwd":
        return [("bias%d-relu%d" % (hb, relu), dict(bias=bias if hb else None, relu=relu), dict(bias=bias if hb else None, relu=bool(relu)))
                for hb in (1, 0) for relu in (1, 0)]
    if kind == "bwd_data":
        return [("relu_src", dict(relu_src=src), dict(mask_src=src)), ("plain", {}, {})]
    return [("db", dict(want_db=True), {}), ("no-db", {}, {})]


def check_db(case, r, a, O):
    """a = dy[M][O]; db within 1 ulp of the float32 rounding of the fp64 column sum."""
    want = a.double().sum(0).float()
    ulps = ulp_distance(r.db, want)
    print("MEASURED|%s|db ulp|%d|1" % (case, ulps))
    assert ulps <= 1, "db is %d ulp from the rounded fp64 column sum" % ulps


SHAPE_KINDS = [(shape, kind) for shape, _ in gd.CASES for kind in gd.KINDS]


def _id(shape, kind):
    return "%s-%s" % ("x".join(str(v) for v in shape), kind)


@pytest.mark.parametrize("shape,kind", SHAPE_KINDS, ids=[_id(s, k) for s, k in SHAPE_KINDS])
def test_fc_every_path(request, shape, kind):
    """Every case of gemm_dispatch.CASES through every epilogue variant: dispatch row, workspace footprint, accuracy rule,
    exact epilogue semantics, stale-workspace determinism and the workspace contract (a), (b), (c)."""
    case = request.node.name
    L = product_lib()
    M, I, O = shape
    g = gd.fc_gemm(kind, M, I, O)
    p = gd.fc_plan(kind, M, I, O)
    assert (p.tile, p.splits, p.live, p.tail) == dict(gd.CASES)[shape][kind], "gemm_dispatch.CASES disagrees with the restated rules"
    assert L.clhip_fc_ws(M, I, O) >= p.need_bytes                                           # contract (c)
    a, b, Av, Bv = operands(kind, shape)
    ref = reference(kind, shape)
    need = p.need_bytes // 4
    touched = g.M * g.N * p.splits if p.splits > 1 else 0
    assert touched == need
    outs = {}
    for name, kw, acc in variants(kind, shape):
        r = run_fc(L, kind, shape, a, b, ws_floats=need + WS_SLACK, **kw)
        assert r.rc == 0 and r.clean, "%s: rc %d, gaps or inputs changed: %s" % (name, r.rc, not r.clean)
        check_ws(r, touched, name)
        accuracy(case, name, r.out, ref, g.K, p.splits, **acc)
        outs[name] = r.out
        if kw.get("want_db"):
            check_db(case, r, a, O)
        elif r.db is not None:
            assert all_bits(r.db, OUT_BITS), "db = NULL: the db-sized slot must keep its sentinel"
        if p.splits > 1:                        # stale workspace: a second call on a refilled workspace gives the same bits
            r2 = run_fc(L, kind, shape, a, b, ws_floats=need + WS_SLACK, **kw)
            assert bool(torch.isfinite(r2.out).all()) and bitwise_equal(r.out, r2.out), name + ": two calls differ"
    # exact epilogue semantics, from the variants' outputs
    if kind == "fwd":
        for hb in (1, 0):
            assert torch.equal(outs["bias%d-relu1" % hb], outs["bias%d-relu0" % hb].clamp(min=0)), "relu is not max(v, 0) of the same v"
    elif kind == "bwd_data":
        src = epilogue_inputs(kind, shape)[1].reshape(-1)
        on = src > 0
        assert bitwise_equal(outs["relu_src"][on], outs["plain"][on]), "relu_src > 0 must pass the value through unchanged"
        assert all_bits(outs["relu_src"][~on], 0), "relu_src of 0.0, -0.0 or below must give exactly 0.0 (strict > 0)"
    else:
        assert bitwise_equal(outs["db"], outs["no-db"]), "dw must not depend on db being asked for"
    # workspace contract on the richest variant
    name, kw, acc = variants(kind, shape)[0]
    if p.splits > 1:
        exact = run_fc(L, kind, shape, a, b, ws_floats=need, **kw)                                # (a) exactly the need
        assert exact.rc == 0 and exact.clean and bitwise_equal(exact.out, outs[name]), "(a) ws_bytes = need"
        check_ws(exact, need, "(a)")
        p1 = gd.fc_plan(kind, M, I, O, ws_bytes=p.need_bytes - 1)
        assert p1.splits == 1 and p1.tile == p.tile and p1.k_per_split >= g.K
        for what, extra in (("(b) ws_bytes = need - 1", dict(ws_bytes=p.need_bytes - 1)), ("(b) ws = NULL", dict(ws_null=True))):
            fb = run_fc(L, kind, shape, a, b, ws_floats=need + WS_SLACK, **extra, **kw)       # the slot itself is large enough
            assert fb.rc == 0 and fb.clean, what
            check_ws(fb, 0, what)
            accuracy(case, what, fb.out, ref, g.K, 1, **acc)
    else:
        nows = run_fc(L, kind, shape, a, b, ws_floats=0, ws_null=True, **kw)
        assert nows.rc == 0 and nows.clean and bitwise_equal(nows.out, outs[name]), "one split: the result must not depend on ws"
        check_ws(nows, 0, "ws = NULL")


# --------------------------------------------------------------------------------------------- decline twins
DECLINES = [
    # kind, shape, A one float off, B one float off, why the wide kernel must decline
    ("fwd", (130, 36, 1027), True, False, "A misaligned"), ("fwd", (130, 36, 1027), False, True, "B misaligned"),
    ("fwd", (129, 324, 1025), True, False, "A misaligned"), ("fwd", (129, 324, 1025), False, True, "B misaligned"),
    ("fwd", (130, 38, 1027), False, False, "K & 3"),
    ("bwd_data", (130, 1028, 132), True, False, "A misaligned"), ("bwd_data", (130, 1028, 132), False, True, "B misaligned"),
    ("bwd_data", (132, 1028, 260), True, False, "A misaligned"), ("bwd_data", (132, 1028, 260), False, True, "B misaligned"),
    ("bwd_data", (130, 1028, 38), False, False, "K & 3"),
    ("bwd_data", (130, 1026, 132), False, False, "N & 3 (B rows contiguous along n)"),
    ("bwd_weight", (132, 1028, 260), True, False, "A misaligned"), ("bwd_weight", (132, 1028, 260), False, True, "B misaligned"),
    ("bwd_weight", (260, 1024, 128), True, False, "A misaligned"), ("bwd_weight", (260, 1024, 128), False, True, "B misaligned"),
    ("bwd_weight", (38, 1028, 260), False, False, "K & 3"),
    ("bwd_weight", (132, 1028, 258), False, False, "M & 3 (A rows contiguous along m)"),
    ("bwd_weight", (132, 1026, 260), False, False, "N & 3 (B rows contiguous along n)"),
]


@pytest.mark.parametrize("kind,shape,mis_a,mis_b,why", DECLINES,
                         ids=["%s-%s" % (_id(d[1], d[0]), d[4].split(" (")[0].replace(" & 3", "mod4").replace(" ", "")) for d in DECLINES])
def test_wide_kernel_declines(request, kind, shape, mis_a, mis_b, why):
    """Twins of the wide cases that wide_ok must turn down: same size class, predicted 64x64 with choose_splits' count."""
    L = product_lib()
    M, I, O = shape
    g = gd.fc_gemm(kind, M, I, O)
    assert g.M >= gd.WT and g.N >= 8 * gd.WT, "the twin must be wide by size"
    if mis_a or mis_b:
        assert gd.plan(g).tile == "wide", "aligned, this shape is wide"
    p = gd.plan(g, a_aligned=not mis_a, b_aligned=not mis_b)
    assert p.tile == "64" and p.splits == gd.choose_splits(g.M, g.N, g.K), why
    a, b, Av, Bv = operands(kind, shape)
    name, kw, acc = variants(kind, shape)[0]
    need = p.need_bytes // 4
    r = run_fc(L, kind, shape, a, b, ws_floats=need + WS_SLACK, mis_a=mis_a, mis_b=mis_b, **kw)
    assert r.rc == 0 and r.clean
    check_ws(r, need, why)
    accuracy(request.node.name, name, r.out, reference(kind, shape), g.K, p.splits, **acc)
    if kw.get("want_db"):
        check_db(request.node.name, r, a, O)


# --------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("M", [1, 15, 16, 17, 200])
def test_colsum_rounds_once(request, M):
    """db over the row-group edges of colsum_kernel (per = ceil(M / 16): at M = 17 per is 2 and the groups from 9 on are
    empty) and its column-block edges (16 columns per block)."""
    L = product_lib()
    I = 3
    for O in (1, 16, 17, 33):
        shape = (M, I, O)
        a, b, Av, Bv = operands("bwd_weight", shape, seed=5)
        r = run_fc(L, "bwd_weight", shape, a, b, want_db=True)
        assert r.rc == 0 and r.clean
        check_db("%s[O=%d]" % (request.node.name, O), r, a, O)
        n = run_fc(L, "bwd_weight", shape, a, b, want_db=False)
        assert n.rc == 0 and n.clean and all_bits(n.db, OUT_BITS) and bitwise_equal(n.out, r.out), "db = NULL"


# --------------------------------------------------------------------------------------------- row and column isolation
ISOLATION = [("fwd", (65, 500, 65)), ("bwd_data", (130, 36, 1027)), ("bwd_weight", (200, 128, 20)),             # 64x64 tiles
             ("fwd", (129, 324, 1025)), ("bwd_data", (132, 1028, 260)), ("bwd_weight", (260, 1024, 128))]      # wide, one per layout


@pytest.mark.parametrize("kind,shape", ISOLATION, ids=[_id(s, k) for k, s in ISOLATION])
def test_non_finite_stays_in_its_row_or_column(kind, shape):
    """One +inf (then one NaN) in A(m*, k*) reaches output row m* only; one in B(k*, n*) reaches output column n* only.
    In terms of the entry points' tensors (logical views of operands()):
      fwd         A(m,k) = x[m][k]  -> row m of y;       B(k,n) = w[n][k] -> column n of y  (output feature n)
      bwd_data    A(m,k) = dy[m][k] -> row m of dx;      B(k,n) = w[k][n] -> column n of dx (input feature n)
      bwd_weight  A(m,k) = dy[k][m] -> row m of dw (output feature m);  B(k,n) = x[k][n] -> column n of dw
    Every case here is split over K, so the slabs and the reduce kernel are covered too; the other operand has no zero, so the
    poisoned row / column is non-finite everywhere."""
    L = product_lib()
    g = gd.fc_gemm(kind, *shape)
    p = gd.plan(g)
    assert p.splits > 1 and p.tile == ("64" if (kind, shape) in ISOLATION[:3] else "wide")
    need = p.need_bytes // 4
    a, b, Av, Bv = operands(kind, shape)
    assert bool((Av != 0).all()) and bool((Bv != 0).all())
    clean = run_fc(L, kind, shape, a, b, ws_floats=need + WS_SLACK)
    assert clean.rc == 0 and clean.clean and bool(torch.isfinite(clean.out).all())
    clean_out = clean.out.view(g.M, g.N)
    ms, ns, ks = g.M - 1, g.N - 1, g.K - 1                 # the ragged last row / column, the last (shallow) live split
    for val in (float("inf"), float("nan")):
        for which in ("A", "B"):
            a2, b2, Av2, Bv2 = operands(kind, shape)
            if which == "A":
                Av2[ms, ks] = val
            else:
                Bv2[ks // 2, ns] = val
            r = run_fc(L, kind, shape, a2, b2, ws_floats=need + WS_SLACK)
            assert r.rc == 0 and r.clean
            out = r.out.view(g.M, g.N)
            keep = torch.ones((g.M, g.N), dtype=torch.bool)
            if which == "A":
                keep[ms, :] = False
            else:
                keep[:, ns] = False
            assert bitwise_equal(out[keep], clean_out[keep]), "%s in %s leaked out of its %s" % (val, which, "row" if which == "A" else "column")
            assert not bool(torch.isfinite(out[~keep]).any()), "%s in %s did not reach all of its %s" % (val, which, "row" if which == "A" else "column")


# --------------------------------------------------------------------------------------------- wide versus 64x64, bitwise
@pytest.fixture(scope="module")
def nowide_lib():
    """libclhip_nowide.so: gemm.hip compiled with CLHIP_NO_WIDE_GEMM (wide_ok always false), loaded next to the product library.
    Rebuilt when the fingerprint of gemm.hip, the headers and the flags changes."""
    from clsurvey_amd import _lib, build
    L = _lib.lib()                                   # maps torch's HIP runtime first (see _lib.lib)
    out = os.path.join(build.HERE, "libclhip_nowide.so")
    stamp = out + ".sha256"
    try:
        import glob
        hdrs = sorted(glob.glob(os.path.join(build.CSRC, "*.hpp"))) + [os.path.join(build.HERE, "..", "include", "clhip.h")]
        want = build._fingerprint([os.path.join(build.CSRC, "gemm.hip")] + hdrs, build.FLAGS + ["-DCLHIP_NO_WIDE_GEMM"])
        have = open(stamp).read().strip() if os.path.exists(stamp) and os.path.exists(out) else ""
        if have != want:
            assert build.build_variant("nowide", "gemm.hip", ["CLHIP_NO_WIDE_GEMM"], verbose=False) == out
            with open(stamp, "w") as f:
                f.write(want + "\n")
    except Exception as e:                           # no compiler or a read-only tree where the tests run
        pytest.skip("build_variant('nowide') cannot run here: %r" % (e,))
    h = C.CDLL(os.path.abspath(out))
    for name in list(ENTRY.values()) + ["clhip_fc_ws"]:
        fn, src = getattr(h, name), getattr(L, name)
        fn.restype, fn.argtypes = src.restype, src.argtypes
    return h


WIDE = [(shape, kind) for shape, row in gd.CASES for kind in gd.KINDS if row[kind][0] == "wide"]


@pytest.mark.parametrize("shape,kind", WIDE, ids=[_id(s, k) for s, k in WIDE])
def test_wide_tile_equals_64_tile_bitwise(request, nowide_lib, shape, kind):
    """The comment above gemm_wide_kernel: same k order per output element inside a split.  Where both split rules give the
    same count the split ranges are the same too (k_per_split depends on K and the count alone), so the two kernels must
    agree bit for bit; where the counts differ only the accuracy rule holds for each."""
    L = product_lib()
    M, I, O = shape
    g = gd.fc_gemm(kind, M, I, O)
    p = gd.fc_plan(kind, M, I, O)
    s64 = gd.choose_splits(g.M, g.N, g.K)
    assert p.tile == "wide" and p.splits == gd.choose_splits_wide(g.M, g.N, g.K)
    if g.K < 192:
        assert p.splits == 1 and s64 == 1
    a, b, Av, Bv = operands(kind, shape)
    ref = reference(kind, shape)
    floats = g.M * g.N * max(p.splits, s64) + WS_SLACK
    for name, kw, acc in variants(kind, shape):
        rw = run_fc(L, kind, shape, a, b, ws_floats=floats, **kw)
        rn = run_fc(nowide_lib, kind, shape, a, b, ws_floats=floats, **kw)
        assert rw.rc == 0 and rn.rc == 0 and rw.clean and rn.clean
        check_ws(rw, g.M * g.N * p.splits if p.splits > 1 else 0, "wide")
        check_ws(rn, g.M * g.N * s64 if s64 > 1 else 0, "64x64")
        accuracy(request.node.name, name + " wide", rw.out, ref, g.K, p.splits, **acc)
        accuracy(request.node.name, name + " 64x64", rn.out, ref, g.K, s64, **acc)
        if p.splits == s64:
            assert bitwise_equal(rw.out, rn.out), "%s: wide and 64x64 tiles differ by up to %d ulp" % (name, ulp_distance(rw.out, rn.out))
