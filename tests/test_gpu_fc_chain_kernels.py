"""Kernel-level parity of csrc/fc_chain.hip (fc_tail_kernel, fc_chain_wgrad_kernel, fc_bwd_combo_kernel) through a NetEngine
over the TINY convolution front of test_gpu_parity.py: 32x32 input (flattened width 128: the first Linear layer runs unsplit,
the tail reads h1 from the activation workspace) and 64x64 input (width 512: the first Linear layer is split over K and the
tail sums its slabs itself — with d1 != 128 in the general eight-slabs-per-trip loop).

Which loop a case takes.  K1 = d1 rounded up to 32.  (128, 128, 32), (100, 36, 7) and (124, 128, 31) have K1 = 128: the 128-wide slab
loop, with rows of 100 / 124 floats in two of them.  (96, 64, 20) and (4, 4, 2) have K1 = 96 / 32: the general slab loop, eight
slabs per trip; at 64x64 choose_splits gives at most 5 splits (4 live slabs), so one more case runs (96, 64, 20) on 128x128
input (flattened width 2048, 16 live slabs: a second trip).  The weight-gradient launch holds every load in flight up to a
batch of 256 and runs a double buffer above it: 255, 256, 257, 289, 1024 sit on both sides.  Every batch runs at
(100, 36, 7) and, up to 289, at (96, 64, 20) on 64x64; every other case runs 1, 33 and 289.

(a) Bitwise.  clhip_net_layer_paths' new bits are asserted first: the fused plan says fc_tail for Linear 2 and 3 and fc_fused for
all three, the CLHIP_FC_TAIL=0 plan says fc_tail for none — otherwise the comparison would be the per-layer path with itself.
Then logits, loss, stats and the WHOLE gradient arena are compared bit for bit, for ce_mean / ce_sum, all classes and a slice
that starts at a nonzero column, the evaluation call and the forward-only call, and h1 / h2 as the activation workspace holds
them.  test_tail_steps_aside_and_says_so: max_batch = 1025, 40 classes, CLHIP_FC_TAIL=0 and a Dropout whose mask is set (training
mode) clear the bit; the twin without that one property sets it.

(b) Weight gradients, per element (u = 2^-24).  dW_l[o][i] = sum_n dz_l[n][o] h_{l-1}[n][i] is a float32 dot product over the batch:
any summation order is within gamma_N ~ N u of the exact value of ITS inputs, (N + 3) u (|dz_l|^T |h_{l-1}|)[o][i] with the slack for
the zero padding to 32 samples and the stores that test_gpu_gemm_kernels.py uses.  The inputs h0, h1, h2 are read back from the
device (layer_input) and the ReLU masks are taken from them, so both sides share them exactly; dz_3 is the dlogits the test hands to
backward(), also exact.  The device's dz_2 and dz_1 are float32 products themselves: dz_l = (dz_{l+1} W_{l+1}) . [h_l > 0] carries
e_l = ((K + 3) u |dz_{l+1}| + e_{l+1}) |W_{l+1}| under the mask (K = width of dz_{l+1}, e_3 = 0, first order), which reaches dW_l as
e_l^T |h_{l-1}| and db_l as sum_n e_l.  Asserted: |dev - fp64| <= (N + 3) u |dz_l|^T |h_{l-1}| + e_l^T |h_{l-1}| and
|db_dev - fp64| <= (N + 3) u sum_n |dz_l| + sum_n e_l; torch's float32 CPU chain on the same values has to meet both (a condition on the
inputs).  A second backward gives the same bits; the arena starts from a sentinel and every element outside a parameter's slot
keeps it (the padding behind a 7-, 31- or 2-wide bias is where a db write one too far would land); the saved activations are
unchanged.

(c) test_path_bits_envelope (no GPU): plans through the C ABI; widths that are no multiple of 4, widths above 128, 33 and 40
classes, max_batch 1025 and CLHIP_FC_TAIL=0 clear fc_tail and keep fc_fused; 4096 tiles keep fc_fused, more clear it.  The tail's
arrival counter is device memory, so a plan made without a device never has fc_tail set: there the clear cases hold trivially
and the set ones are asserted only where a device exists (this test runs on the GPU machine too, and (a) asserts them as well).

Measured on one MI355X (worst element over the batches of a case: device / bound, float32 CPU / bound; every check prints
`MEASURED|case|what|device/bound|float32 CPU/bound` before it asserts, run with -s).  The single sample is one rounding of
one product, 1 / (N + 3) = 0.25 of the bound by construction, hence the second pair of columns:
  (d1, d2, classes)-input    dW, all batches   db, all batches    dW, batch > 1     db, batch > 1
  128x128x32-32              0.243 / 0.243     0.035 / 0.035      0.066 / 0.066     0.018 / 0.019
  128x128x32-64              0.247 / 0.247     0.050 / 0.050      0.071 / 0.071     0.018 / 0.019
  96x64x20-32                0.241 / 0.241     0.075 / 0.045      0.055 / 0.055     0.028 / 0.021
  96x64x20-64                0.239 / 0.239     0.052 / 0.059      0.105 / 0.105     0.052 / 0.052
  100x36x7-32                0.200 / 0.200     0.142 / 0.117      0.045 / 0.055     0.034 / 0.015
  100x36x7-64                0.245 / 0.245     0.122 / 0.144      0.154 / 0.154     0.045 / 0.058
  4x4x2-32                   0.101 / 0.185     0.051 / 0.127      0.039 / 0.050     0.013 / 0.026
  4x4x2-64                   0.135 / 0.135     0.067 / 0.067      0.041 / 0.052     0.017 / 0.013
  124x128x31-32              0.243 / 0.243     0.039 / 0.039      0.080 / 0.080     0.029 / 0.014
  124x128x31-64              0.244 / 0.244     0.041 / 0.041      0.075 / 0.075     0.029 / 0.016
  96x64x20-128 (batch 33)    0.044 / 0.044     0.028 / 0.021
  100x36x7-64 by batch (dW; db):  1: 0.245; 0.122   15: 0.154; 0.045   16: 0.088; 0.027   17: 0.081; 0.036   33: 0.057; 0.034
                                  200: 0.028; 0.011   255: 0.024; 0.005   256: 0.023; 0.006   257: 0.033; 0.009   289: 0.045; 0.007
                                  1024: 0.023; 0.002
  (a): 0 differing elements in all 46 (case, batch) pairs.
  Run time on the MI355X: 24 tests in 4.1 s; 1.05 s for the first (library load, first plans), at most 0.18 s for any other.

Mutation check, run once against scratch copies of fc_chain.hip (each mutant only skips reads, none writes elsewhere; one run of
this file per mutant with CLHIP_LIB on the mutant library; not part of the repository):
  (f) the double-buffered wgrad loop (npad > 256) stops      10 fail: weight_gradients_under_the_derived_bound, every case that runs a batch
      one 32-sample chunk early                              above 256 (n = 289 dW1 at 800 .. 28000 times the bound); not [96x64x20-128], batch 33
  (g) the general slab loop reads slabs s < live - 1         4 fail: tail_is_bitwise...[96x64x20-64], [4x4x2-64], [96x64x20-128] (logits differ from
                                                             the per-layer path at the first batch) and weight_gradients...[4x4x2-64] (h1 without its
                                                             last slab leaves the 4-wide net dead: "the reference gradient is all zero").  The
                                                             K1 = 128 cases pass and must: they do not run that loop
  (h) db: the shuffle that adds the odd samples' half is     11 fail: weight_gradients... in every case (n = 33 db1 at 1e4 .. 5e4 times the bound)
      dropped (tot = asum)
"""
import copy
import ctypes as C
import os

import pytest
import torch

import gemm_dispatch as gd
from kernel_parity import bitwise_equal

gpu = pytest.mark.gpu
DEV = "cuda"
TINY = [16, "M", 16, "M", 32, 32, "M", 32, 32, "M"]          # the front of test_gpu_parity.py (asserted below)
FC_FIRST = 6                                                   # six conv layers, then Linear 6, 7, 8
SHAPES = [(128, 128, 32), (96, 64, 20), (100, 36, 7), (4, 4, 2), (124, 128, 31)]       # (d1, d2, classes)
BATCHES = [1, 15, 16, 17, 33, 200, 255, 256, 257, 289, 1024]
U = 2.0 ** -24
SENTINEL = 7.25


def flat_width(hw):
    return 32 * (hw // 16) ** 2


def batches_of(shape, hw):
    """Every batch at (100, 36, 7) on 64x64 (h1 rows of 100 floats padded to K1 = 128: the 128-wide slab loop) and at
    (96, 64, 20) on 64x64 (K1 = 96: the general slab loop; without 1024, which 20 classes put outside the tail); elsewhere the single sample and a ragged batch below and one
    above the 256-sample threshold of the weight-gradient loop."""
    if hw == 128:
        return [33]
    if (shape, hw) == ((96, 64, 20), 64):
        return [n for n in BATCHES if n * (20 | 1) <= 12288]      # (the tail's per-call range: every batch but 1024)
    return BATCHES if (shape, hw) == ((100, 36, 7), 64) else [1, 33, 289]


# 128x128 input (flattened width 2048), one case: 16 live slabs, so the general slab loop (eight per trip) takes a second trip
CASES = [(s, hw) for s in SHAPES for hw in (32, 64)] + [((96, 64, 20), 128)]
IDS = ["%dx%dx%d-%d" % (s + (hw,)) for s, hw in CASES]


def make_model(hw, shape, dropout=False, seed=0):
    from clsurvey_amd import models
    d1, d2, ncls = shape
    torch.manual_seed(seed + d1 + 3 * d2 + 7 * ncls + hw)
    m = models.VGGSlim(cfg=TINY, num_classes=ncls, classifier_inputdim=flat_width(hw), classifier_dim1=d1, classifier_dim2=d2,
                       dropout=dropout)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
            torch.nn.init.normal_(mod.bias, std=0.1)
    return m


def make_engine(model, max_batch, hw, tail=True):
    """CLHIP_FC_TAIL is read when the plan is created."""
    from clsurvey_amd.net import NetEngine
    old = os.environ.get("CLHIP_FC_TAIL")
    os.environ["CLHIP_FC_TAIL"] = "1" if tail else "0"
    try:
        return NetEngine(model, max_batch, (3, hw, hw), DEV)
    finally:
        if old is None:
            del os.environ["CLHIP_FC_TAIL"]
        else:
            os.environ["CLHIP_FC_TAIL"] = old


def path_bits(eng):
    """({layer: fc_tail}, {layer: fc_fused}) of the three Linear layers."""
    p = {li: eng.layer_paths(li) for li in (FC_FIRST, FC_FIRST + 1, FC_FIRST + 2)}
    return {li: v["fc_tail"] for li, v in p.items()}, {li: v["fc_fused"] for li, v in p.items()}


def assert_split(n, hw, d1):
    """64x64: the first Linear layer runs in at least 2 splits, so the tail gets slabs; 32x32: unsplit."""
    s = gd.choose_splits(n, d1, flat_width(hw))
    assert (s >= 2) if hw >= 64 else (s == 1), (n, hw, d1, s)
    if hw == 128:
        assert gd.plan(gd.fc_gemm("fwd", n, flat_width(hw), d1)).live > 8 and (d1 + 31) // 32 * 32 != 128
    return s


def inputs(n, hw, ncls, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, hw, hw, generator=g).to(DEV), torch.randint(0, ncls, (n,), generator=g).to(DEV)


# ---------------------------------------------------------------------------------------------------- (a) bitwise
@gpu
@pytest.mark.parametrize("shape,hw", CASES, ids=IDS)
def test_tail_is_bitwise_the_per_layer_path(request, shape, hw):
    """Logits, loss, stats and the whole gradient arena of the fused tail against a plan created with CLHIP_FC_TAIL=0, for
    ce_mean / ce_sum, all classes and a slice that starts at a nonzero column, and the forward-only call."""
    from test_gpu_parity import TINY as PARITY_TINY
    assert PARITY_TINY == TINY
    d1, d2, ncls = shape
    ns = batches_of(shape, hw)
    model = make_model(hw, shape)
    fused, plain = make_engine(model, max(ns), hw, True), make_engine(copy.deepcopy(model), max(ns), hw, False)
    tail, wg = path_bits(fused)
    assert tail == {FC_FIRST: False, FC_FIRST + 1: True, FC_FIRST + 2: True} and all(wg.values()), "the fused tail did not take this plan"
    tail, wg = path_bits(plain)
    assert not any(tail.values()) and all(wg.values())
    for n in ns:
        assert n * (ncls | 1) <= 12288, "outside the tail's per-call range"
        splits = assert_split(n, hw, d1)
        x, y = inputs(n, hw, ncls, 5 + n)
        worst = 0
        for kind in ("ce_mean", "ce_sum"):
            for sl in (None, (ncls // 2, ncls)):
                out = []
                for eng in (fused, plain):
                    st = torch.zeros(2, dtype=torch.float64, device=DEV)
                    eng.arena.grad.zero_()
                    loss, logits = eng.loss_step(x, y if sl is None else y % (sl[1] - sl[0]), kind, backward=True, stats=st,
                                                 want_logits=True, class_slice=sl)
                    torch.cuda.synchronize()
                    out.append((loss.clone(), logits.clone(), eng.arena.grad.clone(), st.clone()))
                (l0, z0, g0, s0), (l1, z1, g1, s1) = out
                diff = int((z0 != z1).sum()) + int((g0 != g1).sum()) + int((l0 != l1).sum()) + int((s0 != s1).sum())
                worst = max(worst, diff)
                # (a slice of one class has softmax 1 and no gradient at all: 2 classes, slice [1, 2))
                assert bool(torch.isfinite(g0).all()) and (float(g0.abs().max()) > 0 or (sl is not None and sl[1] - sl[0] == 1))
                assert bitwise_equal(z0, z1), (n, kind, sl, "logits")
                assert bitwise_equal(l0, l1) and torch.equal(s0, s1), (n, kind, sl, l0, l1, s0, s1)
                assert bitwise_equal(g0, g1), (n, kind, sl, float((g0 - g1).abs().max()))
        st0, st1 = (torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(2))
        la, _ = fused.loss_step(x, y, "ce_mean", backward=False, stats=st0)
        la = la.clone()
        lb, _ = plain.loss_step(x, y, "ce_mean", backward=False, stats=st1)
        assert bitwise_equal(la, lb) and torch.equal(st0, st1), (n, "evaluation")
        za, zb = fused.forward(x), plain.forward(x)
        worst = max(worst, int((za != zb).sum()))
        print("MEASURED|%s|n=%d splits=%d differing elements|%d|0" % (request.node.name, n, splits, worst))
        assert bitwise_equal(za, zb), (n, "forward only")
        for li in (FC_FIRST + 1, FC_FIRST + 2):          # h1, h2 as the weight-gradient launch will read them
            assert bitwise_equal(fused.layer_input(li, n), plain.layer_input(li, n)), (n, li)


@gpu
def test_tail_steps_aside_and_says_so():
    """max_batch = 1025, 40 classes, a Dropout in the classifier (training mode: a mask is set): the path bit is clear, and
    it is set for the twin that differs in that one respect."""
    def tail_bits(eng):
        return [path_bits(eng)[0][li] for li in (FC_FIRST, FC_FIRST + 1, FC_FIRST + 2)]
    shape = (128, 128, 32)
    assert tail_bits(make_engine(make_model(32, shape), 1024, 32)) == [False, True, True]
    assert tail_bits(make_engine(make_model(32, shape), 1025, 32)) == [False, False, False]
    assert tail_bits(make_engine(make_model(32, (128, 128, 40)), 16, 32)) == [False, False, False]
    assert tail_bits(make_engine(make_model(32, shape), 16, 32, tail=False)) == [False, False, False]
    m = make_model(32, shape, dropout=True)
    eng = make_engine(m, 16, 32)
    x, y = inputs(16, 32, 32, 3)
    m.eval()
    eng.loss_step(x, y, "ce_mean", backward=True)
    assert tail_bits(eng) == [False, True, True], "evaluation mode: no mask is set, the tail runs"
    m.train()
    eng.loss_step(x, y, "ce_mean", backward=True)
    assert tail_bits(eng) == [False, False, False], "training mode: the masks of the Dropout modules are set"
    assert all(path_bits(eng)[1].values())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- (b) weight gradients
def chain_reference(h, dlogits, Ws, dtype):
    """dz_l, dW_l, db_l (l = 1, 2, 3) from the device's own activations h = [h0, h1, h2]: the ReLU masks are (h1 > 0), (h2 > 0)
    as read back, so a near-tie cannot split the two sides."""
    h = [t.to(dtype) for t in h]
    W = [w.to(dtype) for w in Ws]
    dz = [None, None, dlogits.to(dtype)]
    dz[1] = (dz[2] @ W[2]) * (h[2] > 0)
    dz[0] = (dz[1] @ W[1]) * (h[1] > 0)
    return dz, [dz[l].t() @ h[l] for l in range(3)], [dz[l].sum(0) for l in range(3)]


def chain_bounds(h, dz64, Ws, n):
    """Per element: |dW_l| error <= (N + 3) u (|dz_l|^T |h_{l-1}|) + e_l^T |h_{l-1}|, |db_l| error <= (N + 3) u sum_n |dz_l| + sum_n e_l,
    where e_l bounds the error of the device's dz_l: e_3 = 0 (dlogits is given), e_l = ((K + 3) u |dz_{l+1}| + e_{l+1}) |W_{l+1}|
    under the mask, K = the width of dz_{l+1} (first order: |dz| is taken from the fp64 chain)."""
    a = [t.double().abs() for t in h]
    W = [w.double().abs() for w in Ws]
    e = [None, None, torch.zeros_like(dz64[2])]
    for l in (1, 0):
        K = dz64[l + 1].shape[1]
        e[l] = (((K + 3) * U * dz64[l + 1].abs() + e[l + 1]) @ W[l + 1]) * (a[l + 1] > 0)
    bw = [(n + 3) * U * (dz64[l].abs().t() @ a[l]) + e[l].t() @ a[l] for l in range(3)]
    bb = [(n + 3) * U * dz64[l].abs().sum(0) + e[l].sum(0) for l in range(3)]
    return bw, bb


def ratio(got, want, bound):
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound.clamp(min=torch.finfo(torch.float64).tiny)).max())


@gpu
@pytest.mark.parametrize("shape,hw", CASES, ids=IDS)
def test_weight_gradients_under_the_derived_bound(request, shape, hw):
    """forward(x), backward(x, dlogits) with a dlogits of the test's own; dW_l / db_l of the three Linear layers from the
    arena against fp64 on the float32 values the device holds (h0, h1, h2 through layer_input)."""
    d1, d2, ncls = shape
    ns = batches_of(shape, hw)
    model = make_model(hw, shape, seed=1)
    eng = make_engine(model, max(ns), hw)
    assert all(path_bits(eng)[1].values()), "the fused weight-gradient launch did not take this plan"
    lin = [m for m in model.classifier if isinstance(m, torch.nn.Linear)]
    A = eng.arena
    slots = [A.slot(p) for m in lin for p in (m.weight, m.bias)]
    owned = torch.zeros(A.numel, dtype=torch.bool)
    for p in A.params:
        o, k = A.slot(p)
        owned[o:o + k] = True
    Ws = [m.weight.detach().cpu().clone() for m in lin]
    for n in ns:
        assert_split(n, hw, d1)
        x, _ = inputs(n, hw, ncls, 11 + n)
        g = torch.Generator().manual_seed(23 + n)
        dlogits = (torch.randn(n, ncls, generator=g) / n).to(DEV)
        eng.forward(x)
        h = [eng.layer_input(FC_FIRST + l, n).cpu().clone() for l in range(3)]
        runs = []
        for _ in range(2):
            A.grad.fill_(SENTINEL)
            eng.backward(x, dlogits)
            torch.cuda.synchronize()
            runs.append(A.grad.cpu().clone())
        grad = runs[0]
        for o, k in slots:
            assert bitwise_equal(runs[0][o:o + k], runs[1][o:o + k]), (n, "two calls differ")
        assert bool((grad[~owned] == SENTINEL).all()), "an arena element outside every parameter's slot was written"
        for l in range(3):
            assert bitwise_equal(eng.layer_input(FC_FIRST + l, n).cpu(), h[l]), "backward changed a saved activation"
        dz64, dw64, db64 = chain_reference(h, dlogits.cpu(), Ws, torch.float64)
        _, dw32, db32 = chain_reference(h, dlogits.cpu(), Ws, torch.float32)
        bw, bb = chain_bounds(h, dz64, Ws, n)
        for l, m in enumerate(lin):
            gw = A.view("grad", m.weight).cpu()
            gb = A.view("grad", m.bias).cpu()
            assert float(dw64[l].abs().max()) > 0, "layer %d: the reference gradient is all zero, the inputs do not suit the test" % (l + 1)
            for what, got, w64, w32, bound in (("dW%d" % (l + 1), gw, dw64[l], dw32[l], bw[l]), ("db%d" % (l + 1), gb, db64[l], db32[l], bb[l])):
                r_dev, r_cpu = ratio(got, w64, bound), ratio(w32, w64, bound)
                print("MEASURED|%s|n=%d %s|%.3f|%.3f" % (request.node.name, n, what, r_dev, r_cpu))
                assert r_cpu <= 1.0, "%s: torch's float32 CPU chain misses the bound (%.3f): the inputs do not suit the rule" % (what, r_cpu)
                assert r_dev <= 1.0, "n=%d %s: %.3f of the derived bound" % (n, what, r_dev)


# ---------------------------------------------------------------------------------------------------- (c) envelope, no GPU
def _plan(fc, hw=32, max_batch=8, tail_env=None):
    """A plan of the TINY front and the classifier `fc` = (d1, d2, classes), created through the C ABI with parameter offsets
    laid out like ParamArena's (16-byte slots); no device is needed for that.  Returns the path bits of every layer."""
    from clsurvey_amd import _lib
    lib = _lib.lib()
    widths = [v for v in TINY if v != "M"]
    pools = [i + 1 < len(TINY) and TINY[i + 1] == "M" for i, v in enumerate(TINY) if v != "M"]
    descs = (_lib.LayerDesc * (len(widths) + 3))()
    off, cin = 0, 3
    k = 0
    for w, pool in zip(widths, pools):
        d = descs[k]
        d.type, d.cin, d.cout, d.relu, d.pool = 0, cin, w, 1, int(pool)
        d.ksize, d.stride, d.pad = 3, 1, 1
        d.w_off = off
        off += (w * cin * 9 + 3) // 4 * 4
        d.b_off = off
        off += (w + 3) // 4 * 4
        cin = w
        k += 1
    din = flat_width(hw)
    for j, dout in enumerate(fc):
        d = descs[k]
        d.type, d.cin, d.cout, d.relu, d.pool = 1, din, dout, int(j < 2), 0
        d.w_off = off
        off += (dout * din + 3) // 4 * 4
        d.b_off = off
        off += (dout + 3) // 4 * 4
        din = dout
        k += 1
    old = os.environ.get("CLHIP_FC_TAIL")
    if tail_env is not None:
        os.environ["CLHIP_FC_TAIL"] = tail_env
    try:
        h = C.c_void_p()
        assert lib.clhip_net_create(descs, k, max_batch, 3, hw, hw, C.byref(h)) == 0
    finally:
        if tail_env is not None:
            if old is None:
                del os.environ["CLHIP_FC_TAIL"]
            else:
                os.environ["CLHIP_FC_TAIL"] = old
    bits = [lib.clhip_net_layer_paths(h, li) for li in range(k)]
    assert lib.clhip_net_layer_paths(h, k) < 0 and lib.clhip_net_layer_paths(h, -1) < 0
    lib.clhip_net_destroy(h)
    return bits


def _tiles(din, fc):
    t, i = 0, din
    for o in fc:
        t += ((o + 31) // 32) * ((i + 31) // 32)
        i = o
    return t


def test_path_bits_envelope():
    """The envelope behind the two Linear path bits of clhip_net_layer_paths (clhip_internal_fc_tail_ok and
    clhip_internal_fc_chain_ok are not exported).  The tail also needs a device at plan creation (its arrival counter is
    device memory), so on a host without one bit 6 stays clear everywhere and only its clear cases can be told here; with a
    device the positive twins below are set as well.  The fused weight-gradient bit needs none."""
    TAIL, FUSED = 64, 128
    have_dev = torch.cuda.is_available()

    def fc_bits(fc, **kw):
        bits = _plan(fc, **kw)
        assert all(b >= 0 and not (b & (TAIL | FUSED)) for b in bits[:FC_FIRST]), "conv layers carry no Linear path bit"
        assert all(not (b & 63) for b in bits[FC_FIRST:]), "Linear layers carry none of the conv path bits"
        return [bool(b & TAIL) for b in bits[FC_FIRST:]], [bool(b & FUSED) for b in bits[FC_FIRST:]]

    yes = [False, have_dev, have_dev]
    no = [False, False, False]
    for fc in SHAPES + [(128, 128, 1), (4, 128, 32), (128, 4, 32)]:
        for hw in (32, 64):
            assert fc_bits(fc, hw=hw) == (yes, [True] * 3), (fc, hw)
    assert fc_bits((128, 128, 32), max_batch=1024) == (yes, [True] * 3)
    assert fc_bits((128, 128, 32), max_batch=1025) == (no, [True] * 3)
    assert fc_bits((128, 128, 32), tail_env="0") == (no, [True] * 3)
    # widths that are no multiple of 4, widths above 128, 33 classes: the per-layer launches, the fused weight gradient stays
    for fc in ((126, 128, 32), (128, 126, 32), (127, 125, 7), (132, 128, 32), (128, 132, 32), (256, 256, 10), (128, 128, 33), (96, 64, 40)):
        assert fc_bits(fc) == (no, [True] * 3), fc
    # one wave per 32x32 tile: up to 4096 tiles of dW over the three layers
    assert _tiles(128, (1760, 2176, 33)) == 4096
    assert fc_bits((1760, 2176, 33)) == (no, [True] * 3)
    assert fc_bits((1760, 2208, 33)) == (no, [False] * 3)
    assert _tiles(128, (1760, 2208, 33)) > 4096 and _tiles(128, (2048, 2048, 10)) > 4096
    assert fc_bits((2048, 2048, 10)) == (no, [False] * 3)
