"""Kernel-level parity of csrc/bn.hip: clhip_bn_fwd / clhip_bn_bwd in training and eval mode, ReLU on and off, against fp64 on
the CPU from the same float32 inputs (two-pass variance); the float32 comparator of kernel_parity.fp32_chain_check is torch's
own CPU F.batch_norm with autograd.

Shapes (N, C, HW) are the smallest that reach each branch: M = 1 (the running variance cannot be unbiased), HW = 257 / 300 /
1000 (the `e += 256` loops run more than once and end inside a stride), N = 17 and 33 against BN_SPLIT = 16 (image ranges of
unequal length), N < 16 (empty ranges), C = 300 (the finish kernels need a second block).

Bounds.  save_mean, save_invstd, dgamma, dbeta are double sums rounded once: <= 2 ulp from the rounded fp64 value, on inputs
whose sums do not cancel (|sum v| >= 0.1 sum |v| for each of the four sums and every channel, asserted on the CPU).  The
backward takes y, save_mean and save_invstd as inputs, so its fp64 reference masks with that same y (`!(y > 0)` gives zero: no
allowance for flipped ReLU decisions) and normalises with those same float32 statistics.  y, running_mean, running_var and dz
follow the fp32-chain rule with base 1e-6; dz is measured against max(gamma * invstd) * max|dy|, the size of the terms whose
difference it is.  Eval mode: save_mean is bitwise running_mean, save_invstd <= 2 ulp from fp64.  Every output is bitwise
equal between two runs.

Measured on one MI355X (worst over the cases of a test: device / float32 CPU distance from fp64 relative to the scale, or
ulp / bound; every check prints a `MEASURED|...` line before it asserts, run with -s):
  bn_shapes (24 cases): save_mean / save_invstd / dgamma / dbeta ulp               0 / 1 / 1 / 0   (bound 2)
  bn_shapes: y                                                                     1.6e-07 / 1.2e-07
  bn_shapes: running_mean, running_var                                             6.8e-08 / 6.8e-08, 6.4e-08 / 6.4e-08
  bn_shapes: dz                                                                    1.1e-07 / 3.1e-07
  bn_backward_masks_with_the_y_it_is_given: dgamma / dbeta ulp, dz                 1 / 0, 1.0e-07 / 1.1e-07
  bn_null_outputs_and_misaligned_tensors: y, dz                                    9.4e-08 / 7.7e-08, 1.0e-07 / 1.1e-07
  bn_large_offset: save_mean / save_invstd / dgamma / dbeta ulp                    0 / 0 / 0 / 0
  bn_large_offset: y (float32 save_mean: 100 * 2^-24 * invstd 10, on both sides)   1.7e-05 / 1.8e-05
  bn_large_offset: dz                                                              8.6e-08 / 6.3e-08
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_parity import HAT_BASE, Arena, bitwise_equal, fp32_chain_check, ulp_distance

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
EPS32 = float(np.float32(EPS))              # what the kernels add to the variance
MOM32 = float(np.float32(MOM))
NAN_BITS = 0x7fc00000


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from clsurvey_amd import _lib
    return _lib, _lib.lib()


# --------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def inputs(N, C, HW, offset=1.0, spread=1.0, seed=0):
    """z and dy with per-channel offsets so none of the four channel sums cancels; dy leans on xhat so sum dy * xhat does not."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * C + HW + seed)
    ch = torch.arange(C, dtype=torch.float32).view(1, C, 1)
    z = offset * (1 + 0.25 * (ch % 5)) + spread * torch.randn((N, C, HW), generator=gen)
    gamma = 0.75 + 0.5 * torch.rand(C, generator=gen)
    beta = 0.3 * torch.randn(C, generator=gen)
    rm = 0.2 * torch.randn(C, generator=gen)
    rv = 0.5 + 1.5 * torch.rand(C, generator=gen)
    zc = z - z.mean((0, 2), keepdim=True)
    xh = zc / zc.pow(2).mean((0, 2), keepdim=True).sqrt().clamp_min(1e-3)
    dy = (0.5 + 0.1 * (ch % 3)) + 0.8 * xh + 0.3 * torch.randn((N, C, HW), generator=gen)
    return z, gamma, beta, rm, rv, dy


def stats64(z):
    """Two-pass batch statistics in fp64: mean, biased variance, invstd."""
    z64 = z.double()
    mean = z64.mean((0, 2))
    var = (z64 - mean.view(1, -1, 1)).pow(2).mean((0, 2))
    return mean, var, 1.0 / torch.sqrt(var + EPS32)


def fwd64(z, gamma, beta, rm, rv, training, relu):
    """fp64 forward: y, save_mean, save_invstd, running_mean, running_var."""
    N, C, HW = z.shape
    M = N * HW
    if training:
        mean, var, invstd = stats64(z)
        rm2 = (1 - MOM32) * rm.double() + MOM32 * mean
        rv2 = (1 - MOM32) * rv.double() + MOM32 * (var * M / (M - 1) if M > 1 else var)
    else:
        mean, invstd = rm.double(), 1.0 / torch.sqrt(rv.double() + EPS32)
        rm2, rv2 = rm.double(), rv.double()
    y = (z.double() - mean.view(1, C, 1)) * invstd.view(1, C, 1) * gamma.double().view(1, C, 1) + beta.double().view(1, C, 1)
    if relu:
        y = y.clamp_min(0)
    return y, mean, invstd, rm2, rv2


def fwd32(z, gamma, beta, rm, rv, training, relu):
    """torch's float32 CPU forward: y, running_mean, running_var.  torch refuses a training batch of one value per channel;
    there the comparator is the fp64 result rounded to float32."""
    if training and z.shape[0] * z.shape[2] == 1:
        y64, _, _, rm64, rv64 = fwd64(z, gamma, beta, rm, rv, training, relu)
        return y64.float(), rm64.float(), rv64.float()
    rm2, rv2 = rm.clone(), rv.clone()
    y = F.batch_norm(z.unsqueeze(-1), rm2, rv2, gamma, beta, training, MOM, EPS).squeeze(-1)
    return (torch.relu(y) if relu else y), rm2, rv2


def bwd64(dy, y, z, gamma, mean32, invstd32, training, relu):
    """fp64 backward from the float32 inputs the kernel gets: dz, dgamma, dbeta, and the summands of dgamma / dbeta."""
    N, C, HW = z.shape
    M = N * HW
    dyr = dy.double()
    if relu:
        dyr = torch.where(y.double() > 0, dyr, torch.zeros_like(dyr))        # NaN > 0 is False: !(y > 0) gives zero
    xh = (z.double() - mean32.double().view(1, C, 1)) * invstd32.double().view(1, C, 1)
    dbeta, dgamma = dyr.sum((0, 2)), (dyr * xh).sum((0, 2))
    a = (gamma.double() * invstd32.double()).view(1, C, 1)
    if training:
        dz = a * (dyr - dbeta.view(1, C, 1) / M - xh * dgamma.view(1, C, 1) / M)
    else:
        dz = a * dyr
    return dz, dgamma, dbeta, dyr, dyr * xh


def bwd32(dy, y, z, gamma, beta, rm, rv, mean32, invstd32, training, relu):
    """torch's float32 CPU backward of F.batch_norm, fed the gradient already masked with the y the kernel gets (M = 1 in
    training mode: as fwd32)."""
    if training and z.shape[0] * z.shape[2] == 1:
        return tuple(t.float() for t in bwd64(dy, y, z, gamma, mean32, invstd32, training, relu)[:3])
    zt = z.clone().unsqueeze(-1).requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = F.batch_norm(zt, rm.clone(), rv.clone(), gt, bt, training, MOM, EPS)
    dyr = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    out.backward(dyr.unsqueeze(-1))
    return zt.grad.squeeze(-1), gt.grad, bt.grad


def no_cancel(terms, what):
    s, a = terms.sum((0, 2)).abs(), terms.abs().sum((0, 2))
    assert bool((s >= 0.1 * a).all()), "%s: a channel sum cancels (|sum| / sum|.| = %.3f)" % (what, float((s / a.clamp_min(1e-300)).min()))


# --------------------------------------------------------------------------- device runs
def run_fwd(z, gamma, beta, rm, rv, training, relu, mis=False, null_running=False):
    _lib, L = _L()
    N, C, HW = z.shape
    A = Arena()
    kz, kg, kb = A.add(z, mis), A.add(gamma, mis), A.add(beta, mis)
    krm, krv = A.add(rm, mis), A.add(rv, mis)
    ky = A.add(N * C * HW, mis, fill=NAN_BITS)
    km, ki = A.add(C, mis, fill=NAN_BITS), A.add(C, mis, fill=NAN_BITS)
    A.upload(dev())
    assert A.ptr(kz) % 16 == (4 if mis else 0)
    ws = torch.full((L.clhip_bn_ws(C),), 0xCD, dtype=torch.uint8, device=dev())
    _lib.check(L.clhip_bn_fwd(A.ptr(kz), A.ptr(kg), A.ptr(kb), None if null_running else A.ptr(krm), None if null_running else A.ptr(krv),
                              A.ptr(ky), A.ptr(km), A.ptr(ki), N, C, HW, int(training), MOM, EPS, int(relu), ws.data_ptr(), ws.numel(),
                              _stream()), "clhip_bn_fwd")
    torch.cuda.synchronize()
    A.download()
    assert A.gaps_untouched(), "clhip_bn_fwd wrote outside its tensors"
    for k, t in ((kz, z), (kg, gamma), (kb, beta)):
        assert bitwise_equal(A.get(k), t.reshape(-1)), "clhip_bn_fwd modified an input"
    return dict(y=A.get(ky).clone().view(N, C, HW), mean=A.get(km).clone(), invstd=A.get(ki).clone(), rm=A.get(krm).clone(),
                rv=A.get(krv).clone())


def run_bwd(dy, y, z, gamma, mean32, invstd32, training, relu, mis=False, null_grads=False, null_y=False):
    _lib, L = _L()
    N, C, HW = z.shape
    A = Arena()
    kdy, ky, kz, kg = A.add(dy, mis), A.add(y, mis), A.add(z, mis), A.add(gamma, mis)
    km, ki = A.add(mean32, mis), A.add(invstd32, mis)
    kdz = A.add(N * C * HW, mis, fill=NAN_BITS)
    kdg, kdb = A.add(C, mis, fill=NAN_BITS), A.add(C, mis, fill=NAN_BITS)
    A.upload(dev())
    ws = torch.full((L.clhip_bn_ws(C),), 0xCD, dtype=torch.uint8, device=dev())
    _lib.check(L.clhip_bn_bwd(A.ptr(kdy), None if null_y else A.ptr(ky), A.ptr(kz), A.ptr(kg), A.ptr(km), A.ptr(ki), A.ptr(kdz),
                              None if null_grads else A.ptr(kdg), None if null_grads else A.ptr(kdb), N, C, HW, int(training), int(relu),
                              ws.data_ptr(), ws.numel(), _stream()), "clhip_bn_bwd")
    torch.cuda.synchronize()
    A.download()
    assert A.gaps_untouched(), "clhip_bn_bwd wrote outside its tensors"
    for k, t in ((kdy, dy), (ky, y), (kz, z), (kg, gamma), (km, mean32), (ki, invstd32)):
        assert bitwise_equal(A.get(k), t.reshape(-1)), "clhip_bn_bwd modified an input"
    return dict(dz=A.get(kdz).clone().view(N, C, HW), dgamma=A.get(kdg).clone(), dbeta=A.get(kdb).clone())


# --------------------------------------------------------------------------- checks
def ulp_check(case, what, got, want64, bound=2):
    ulps = ulp_distance(got, want64.float())
    print("MEASURED|%s|%s ulp from the rounded fp64 value|%d|%d" % (case, what, ulps, bound))
    assert ulps <= bound, "%s: %d ulp from the rounded fp64 value" % (what, ulps)


def check_fwd(case, out, z, gamma, beta, rm, rv, training, relu, null_running=False):
    y64, mean64, invstd64, rm64, rv64 = fwd64(z, gamma, beta, rm, rv, training, relu)
    y32, rm32, rv32 = fwd32(z, gamma, beta, rm, rv, training, relu)
    if training:
        no_cancel(z.double(), "sum z")
        ulp_check(case, "save_mean", out["mean"], mean64)
    else:
        assert bitwise_equal(out["mean"], rm), "eval mode: save_mean is not running_mean bit for bit"
    ulp_check(case, "save_invstd", out["invstd"], invstd64)
    fp32_chain_check(case, "y", out["y"], y32, y64, HAT_BASE)
    if training and not null_running:
        fp32_chain_check(case, "running_mean", out["rm"], rm32, rm64, HAT_BASE)
        fp32_chain_check(case, "running_var", out["rv"], rv32, rv64, HAT_BASE)
    else:
        assert bitwise_equal(out["rm"], rm) and bitwise_equal(out["rv"], rv), "the running statistics moved"


def check_bwd(case, out, dy, y, z, gamma, beta, rm, rv, mean32, invstd32, training, relu, null_grads=False):
    C = z.shape[1]
    dz64, dg64, db64, t_beta, t_gamma = bwd64(dy, y, z, gamma, mean32, invstd32, training, relu)
    dz32, dg32, db32 = bwd32(dy, y, z, gamma, beta, rm, rv, mean32, invstd32, training, relu)
    no_cancel(t_beta, "sum dyr")
    no_cancel(t_gamma, "sum dyr * xhat")
    if null_grads:
        assert all(bool((out[k].view(torch.int32) == NAN_BITS).all()) for k in ("dgamma", "dbeta"))
    else:
        ulp_check(case, "dgamma", out["dgamma"], dg64)
        ulp_check(case, "dbeta", out["dbeta"], db64)
    scale = float((gamma.double() * invstd32.double()).abs().max()) * float(dy.abs().max())
    fp32_chain_check(case, "dz", out["dz"], dz32, dz64, HAT_BASE, scale=scale)


SHAPES = [(1, 3, 1), (5, 3, 257), (17, 2, 1000), (16, 4, 300), (2, 300, 5), (33, 7, 64)]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_shapes(request, shape, relu, training):
    """Forward, then the backward on the forward's own y, save_mean and save_invstd."""
    case = request.node.name
    z, gamma, beta, rm, rv, dy = inputs(*shape)
    out = run_fwd(z, gamma, beta, rm, rv, training, relu)
    check_fwd(case, out, z, gamma, beta, rm, rv, training, relu)
    back = run_bwd(dy, out["y"], z, gamma, out["mean"], out["invstd"], training, relu)
    check_bwd(case, back, dy, out["y"], z, gamma, beta, rm, rv, out["mean"], out["invstd"], training, relu)


def test_bn_m_equals_one_running_var(request):
    """M = 1: the batch variance is 0 and there is no unbiased form; running_var moves towards 0 exactly as torch's."""
    z, gamma, beta, rm, rv, dy = inputs(1, 3, 1)
    out = run_fwd(z, gamma, beta, rm, rv, True, False)
    assert bitwise_equal(out["mean"], z.reshape(-1)), "the mean of one value is that value"
    keep = torch.tensor(1.0) - torch.tensor(MOM)                             # float32, as the kernel forms 1 - momentum
    assert bitwise_equal(out["rv"], keep * rv), "running_var must move towards the batch variance 0"
    assert bitwise_equal(out["y"].reshape(-1), beta), "(z - mean) is exactly 0"


def crafted_y(y):
    """+0.0, -0.0, a positive denormal, negatives and NaN in every channel; a denormal IS > 0."""
    y = y.clone()
    N, C, HW = y.shape
    special = torch.tensor([0.0, -0.0, 0.0, -1.5, float("nan"), -1e-30], dtype=torch.float32)
    for c in range(C):
        y[0, c, :6] = special
        y[0, c, 2:3] = torch.tensor([1], dtype=torch.int32).view(torch.float32)          # the smallest positive denormal
        y[N - 1, c, HW - 3:] = torch.tensor([float("nan"), -0.0, 7.0])
    return y


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_backward_masks_with_the_y_it_is_given(request, training):
    case = request.node.name
    shape = (5, 3, 257)
    z, gamma, beta, rm, rv, dy = inputs(*shape)
    y64, mean64, invstd64, _, _ = fwd64(z, gamma, beta, rm, rv, training, True)
    y = crafted_y(y64.float())
    mean32, invstd32 = mean64.float(), invstd64.float()
    back = run_bwd(dy, y, z, gamma, mean32, invstd32, training, True)
    check_bwd(case, back, dy, y, z, gamma, beta, rm, rv, mean32, invstd32, training, True)
    if not training:                                                          # dz = gamma * invstd * dyr: exact zeros where !(y > 0)
        dead = ~(y > 0)
        assert bool((back["dz"][dead] == 0).all()) and bool((back["dz"][0, :, 2] != 0).all())
    # relu off: y is not read at all (NULL is accepted) and the mask is gone
    free = run_bwd(dy, y, z, gamma, mean32, invstd32, training, False, null_y=True)
    check_bwd(case + "/linear", free, dy, y, z, gamma, beta, rm, rv, mean32, invstd32, training, False)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_bn_null_outputs_and_misaligned_tensors(request, relu):
    """running_* NULL in training mode, dgamma / dbeta NULL, and every tensor one float past a 16-byte boundary: the same
    bits as the plain run."""
    case = request.node.name
    shape = (5, 3, 257)
    z, gamma, beta, rm, rv, dy = inputs(*shape)
    plain = run_fwd(z, gamma, beta, rm, rv, True, relu)
    check_fwd(case, plain, z, gamma, beta, rm, rv, True, relu)
    nor = run_fwd(z, gamma, beta, rm, rv, True, relu, null_running=True)
    check_fwd(case + "/no-running", nor, z, gamma, beta, rm, rv, True, relu, null_running=True)
    off = run_fwd(z, gamma, beta, rm, rv, True, relu, mis=True)
    for k in ("y", "mean", "invstd"):
        assert bitwise_equal(nor[k], plain[k]) and bitwise_equal(off[k], plain[k]), k
    assert bitwise_equal(off["rm"], plain["rm"]) and bitwise_equal(off["rv"], plain["rv"])
    args = (dy, plain["y"], z, gamma, plain["mean"], plain["invstd"], True, relu)
    b0 = run_bwd(*args)
    check_bwd(case, b0, dy, plain["y"], z, gamma, beta, rm, rv, plain["mean"], plain["invstd"], True, relu)
    b1 = run_bwd(*args, null_grads=True)
    check_bwd(case + "/no-grads", b1, dy, plain["y"], z, gamma, beta, rm, rv, plain["mean"], plain["invstd"], True, relu, null_grads=True)
    b2 = run_bwd(*args, mis=True)
    assert bitwise_equal(b1["dz"], b0["dz"])
    for k in ("dz", "dgamma", "dbeta"):
        assert bitwise_equal(b2[k], b0[k]), k


def test_bn_large_offset(request):
    """Per-channel mean about 100, spread about 0.1: the one-pass variance q / M - mean^2 loses about 20 of its 53 bits.
    Precondition (CPU only): an fp64 emulation of that one-pass formula gives invstd within 1 ulp(float32) of the two-pass value."""
    case = request.node.name
    shape = (16, 4, 300)
    z, gamma, beta, rm, rv, dy = inputs(*shape, offset=100.0, spread=0.1, seed=5)
    mean64, var64, invstd64 = stats64(z)
    assert float(mean64.abs().min()) > 90 and 0.05 < float(var64.sqrt().min()) and float(var64.sqrt().max()) < 0.2
    z64 = z.double().numpy()
    M = shape[0] * shape[2]
    m1 = z64.sum((0, 2)) / M
    v1 = np.maximum((z64 * z64).sum((0, 2)) / M - m1 * m1, 0.0)
    one_pass = torch.from_numpy(1.0 / np.sqrt(v1 + EPS32)).float()
    assert ulp_distance(one_pass, invstd64.float()) <= 1, "the inputs are too hard for the one-pass formula in fp64 itself"
    for relu in (True, False):
        out = run_fwd(z, gamma, beta, rm, rv, True, relu)
        check_fwd(case, out, z, gamma, beta, rm, rv, True, relu)
        back = run_bwd(dy, out["y"], z, gamma, out["mean"], out["invstd"], True, relu)
        check_bwd(case, back, dy, out["y"], z, gamma, beta, rm, rv, out["mean"], out["invstd"], True, relu)


def test_bn_is_bitwise_deterministic():
    shape = (17, 2, 1000)
    z, gamma, beta, rm, rv, dy = inputs(*shape)
    f0 = run_fwd(z, gamma, beta, rm, rv, True, True)
    f1 = run_fwd(z, gamma, beta, rm, rv, True, True)
    for k in f0:
        assert bitwise_equal(f0[k], f1[k]), "forward: %s differs between two runs" % k
    b0 = run_bwd(dy, f0["y"], z, gamma, f0["mean"], f0["invstd"], True, True)
    b1 = run_bwd(dy, f0["y"], z, gamma, f0["mean"], f0["invstd"], True, True)
    for k in b0:
        assert bitwise_equal(b0[k], b1[k]), "backward: %s differs between two runs" % k
