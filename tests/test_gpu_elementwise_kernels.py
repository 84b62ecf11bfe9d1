"""Kernel-level parity of csrc/elementwise.hip, table-driven: one fp64 restatement per entry point (oracle.regularizers_ref
where it has one, evaluated in float64 on the same float32 inputs), the same functions in float32 on the CPU as comparator.

Sizes: 1, 3, 4, 5, 255, 1023; 2048 * 256 + 3 (the scalar path of the capped grid wraps once a pointer is misaligned);
4 * 2048 * 256 + 7 (the float4 path wraps and leaves a tail of 3).  Alignment: for every multi-pointer kernel each pointer in
turn sits one float past a 16-byte boundary, then all of them; every output must equal the all-aligned run bit for bit (the
scalar and the float4 path are the same arithmetic), and the aligned run meets the fp32-chain rule against fp64 (base 1e-6;
1e-5 for SI's w and omega, sums of products of differences).  relu_bwd, the zeroed w / copied init_val of si_consolidate,
imm_merge (against the float32 torch sequence its comment names) and the da of mse_mean are bitwise; the loss of mse_mean is a
double sum rounded once, <= 2 ulp from fp64.  sigmoid (base 1e-5) sees +-100, +-88.7 (around expf's overflow), +-0.0.
Every tensor lives in an arena with sentinel gaps.

Measured on one MI355X (every check prints `MEASURED|<test id>|<what>|<device>|<float32 CPU or bound>` before it asserts, run
with -s; worst over sizes and cases, device / float32 CPU distance from fp64 relative to the tensor's largest entry):
  reg_sgd_step (omega, no omega; first, later): theta, buf                         5.5e-08 / 5.4e-08, 1.4e-07 / 1.4e-07
  si_step (first, later): theta, buf, w                                            5.6e-08 / 5.6e-08, 1.7e-07 / 1.7e-07, 4.8e-07 / 4.3e-07
  si_consolidate: omega                                                            1.5e-07 / 1.5e-07
  fisher_accum, mas_accum: omega                                                   4.0e-08 / 4.0e-08, 7.8e-08 / 7.1e-08
  sigmoid forward, backward                                                        8.9e-08 / 8.9e-08, 9.4e-08 / 9.4e-08
  adadelta_step, three steps: theta, square_avg, acc_delta                         4.6e-08 / 4.6e-08, 1.2e-07 / 3.0e-07, 5.6e-07 / 5.7e-07
  mse_mean: loss ulp from the rounded fp64 mean (bound 2), da ulp (bound 0)        0, 0
  misaligned against aligned runs, relu_bwd, imm_merge: differing elements         0

Two findings of these tests, fixed in csrc/elementwise.hip: reg_sgd_step and si_step gave results one ulp apart on the scalar
and the float4 path (the compiler fused the multiply-adds of one and not of the other; they are fused by hand now, in the float4
path's form), and mode-IMM was up to 7 ulp from the float32 torch sequence (__fmul_rn / __fadd_rn are plain operators that the
compiler contracted into an fma; the merge now runs under `fp contract(off)`).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_parity import HAT_BASE, LOSS_BASE, Arena, bitwise_equal, fp32_chain_check, ulp_distance
from oracle import regularizers_ref as R

pytestmark = pytest.mark.gpu

WRAP = 2048 * 256
N_SCALAR_WRAP = WRAP + 3
N_VEC_WRAP = 4 * WRAP + 7
SIZES = [1, 3, 4, 5, 255, 1023, N_SCALAR_WRAP, N_VEC_WRAP]
MIS_SIZES = [1, 5, 1023, N_SCALAR_WRAP]
NAN_BITS = 0x7fc00000
LAM, LR, MOM = 400.0, 1e-2, 0.9
SI_BASE = 1e-5


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from clsurvey_amd import _lib
    return _lib, _lib.lib()


def run(entry, tensors, order, scalars, n, mis=()):
    """tensors: name -> host float32 tensor; order: the names in the entry point's pointer order (None = a NULL pointer);
    scalars: the arguments between n and the stream.  Returns name -> tensor after the call."""
    _lib, L = _L()
    A = Arena()
    slot = {name: A.add(t, name in mis) for name, t in tensors.items()}
    A.upload(dev())
    for name in tensors:
        assert A.ptr(slot[name]) % 16 == (4 if name in mis else 0)
    ptrs = [A.ptr(slot[name]) if name is not None else None for name in order]
    _lib.check(getattr(L, entry)(*ptrs, n, *scalars, _stream()), entry)
    torch.cuda.synchronize()
    A.download()
    assert A.gaps_untouched(), entry + " wrote outside its tensors"
    return {name: A.get(slot[name]).clone() for name in tensors}


# --------------------------------------------------------------------------- the table
def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed + n % 1000)
    t = dict(theta=torch.randn(n, generator=gen), grad=0.1 * torch.randn(n, generator=gen),
             omega=1e-2 * torch.randn(n, generator=gen).abs(), init=torch.randn(n, generator=gen),
             w=0.01 * torch.randn(n, generator=gen), buf=0.1 * torch.randn(n, generator=gen))
    return t


def _relu_inputs(n, seed):
    gen = torch.Generator().manual_seed(seed + n % 1000)
    y = torch.randn(n, generator=gen)
    special = torch.tensor([0.0, -0.0, 0.0, float("nan"), -1.0, 2.0])
    special[2:3] = torch.tensor([1], dtype=torch.int32).view(torch.float32)        # a positive denormal: > 0
    k = min(n, 6)
    y[:k] = special[:k]
    if n >= 12:
        y[-6:] = special.flip(0)
    return dict(dy=torch.randn(n, generator=gen), y=y, dx=torch.full((n,), float("nan")))


def _cast(t, names, dtype):
    return [t[k].to(dtype) for k in names]


def ref_reg_sgd(t, dtype, first, use_reg):
    th, g, b = _cast(t, ("theta", "grad", "buf"), dtype)
    om, iv = _cast(t, ("omega", "init"), dtype) if use_reg else (None, None)
    th2, b2 = R.reg_sgd_step(th, g, om if use_reg else None, iv if use_reg else None, None if first else b, LAM, LR, MOM, 5e-4, first)
    return dict(theta=th2, buf=b2)


def ref_si_step(t, dtype, first):
    th, g, om, iv, w, b = _cast(t, ("theta", "grad", "omega", "init", "w", "buf"), dtype)
    th2, b2, w2 = R.si_step(th, g, om, iv, w, None if first else b, LAM, LR, MOM, 1e-4, first)
    return dict(theta=th2, buf=b2, w=w2)


def ref_si_cons(t, dtype):
    om, w, th, iv = _cast(t, ("omega", "w", "theta", "init"), dtype)
    o2, w2, i2 = R.si_consolidate(om, w, th, iv, 1e-3)
    return dict(omega=o2, w=w2, init=i2)


OPS = {
    # name: (entry, input maker, tensors used, pointer order, scalars, reference, {output: base or "bitwise"})
    "reg_sgd-first": ("clhip_reg_sgd_step", _inputs, ("theta", "grad", "omega", "init", "buf"), ("theta", "grad", "omega", "init", "buf"),
                      (LAM, LR, MOM, 5e-4, 1), lambda t, d: ref_reg_sgd(t, d, True, True), dict(theta=HAT_BASE, buf=HAT_BASE)),
    "reg_sgd-later": ("clhip_reg_sgd_step", _inputs, ("theta", "grad", "omega", "init", "buf"), ("theta", "grad", "omega", "init", "buf"),
                      (LAM, LR, MOM, 5e-4, 0), lambda t, d: ref_reg_sgd(t, d, False, True), dict(theta=HAT_BASE, buf=HAT_BASE)),
    "plain_sgd-first": ("clhip_reg_sgd_step", _inputs, ("theta", "grad", "buf"), ("theta", "grad", None, None, "buf"),
                        (LAM, LR, MOM, 5e-4, 1), lambda t, d: ref_reg_sgd(t, d, True, False), dict(theta=HAT_BASE, buf=HAT_BASE)),
    "plain_sgd-later": ("clhip_reg_sgd_step", _inputs, ("theta", "grad", "buf"), ("theta", "grad", None, None, "buf"),
                        (LAM, LR, MOM, 5e-4, 0), lambda t, d: ref_reg_sgd(t, d, False, False), dict(theta=HAT_BASE, buf=HAT_BASE)),
    "si_step-first": ("clhip_si_step", _inputs, ("theta", "grad", "omega", "init", "w", "buf"), ("theta", "grad", "omega", "init", "w", "buf"),
                      (LAM, LR, MOM, 1e-4, 1), lambda t, d: ref_si_step(t, d, True), dict(theta=HAT_BASE, buf=HAT_BASE, w=SI_BASE)),
    "si_step-later": ("clhip_si_step", _inputs, ("theta", "grad", "omega", "init", "w", "buf"), ("theta", "grad", "omega", "init", "w", "buf"),
                      (LAM, LR, MOM, 1e-4, 0), lambda t, d: ref_si_step(t, d, False), dict(theta=HAT_BASE, buf=HAT_BASE, w=SI_BASE)),
    "si_consolidate": ("clhip_si_consolidate", _inputs, ("omega", "w", "theta", "init"), ("omega", "w", "theta", "init"),
                       (1e-3,), ref_si_cons, dict(omega=SI_BASE, w="bitwise", init="bitwise")),
    "fisher_accum": ("clhip_fisher_accum", _inputs, ("omega", "grad"), ("omega", "grad"),
                     (8000.0,), lambda t, d: dict(omega=R.fisher_accum(t["omega"].to(d), t["grad"].to(d), 8000.0)), dict(omega=HAT_BASE)),
    "mas_accum": ("clhip_mas_accum", _inputs, ("omega", "grad"), ("omega", "grad"),
                  (600.0, 800.0), lambda t, d: dict(omega=R.mas_accum(t["omega"].to(d), t["grad"].to(d), 3, 200)), dict(omega=HAT_BASE)),
    "relu_bwd": ("clhip_relu_bwd", _relu_inputs, ("dy", "y", "dx"), ("dy", "y", "dx"),
                 (), lambda t, d: dict(dx=torch.where(t["y"] > 0, t["dy"], torch.zeros_like(t["dy"])).to(d)), dict(dx="bitwise")),
}


@pytest.mark.parametrize("op", list(OPS))
def test_elementwise_parity_and_alignment(request, op):
    case = request.node.name
    entry, make, used, order, scalars, ref, outputs = OPS[op]
    for n in SIZES:
        full = make(n, 17)
        t = {k: full[k] for k in used}
        aligned = run(entry, t, order, scalars, n)
        r32, r64 = ref(t, torch.float32), ref(t, torch.float64)
        for name in used:
            if name not in outputs:
                assert bitwise_equal(aligned[name], t[name]), "%s modified its input %s (n = %d)" % (entry, name, n)
            elif outputs[name] == "bitwise":
                assert bitwise_equal(aligned[name], r32[name]), "%s: %s differs from the float32 reference (n = %d)" % (entry, name, n)
            else:
                fp32_chain_check(case, "%s n = %d" % (name, n), aligned[name], r32[name], r64[name], outputs[name])
        if n not in MIS_SIZES:
            continue
        for mis in [(k,) for k in used] + [tuple(used)]:
            got = run(entry, t, order, scalars, n, mis)
            for name in used:
                assert bitwise_equal(got[name], aligned[name]), \
                    "%s, n = %d: %s differs from the aligned run when %s is off a 16-byte boundary" % (entry, n, name, " and ".join(mis))


def test_relu_bwd_special_values():
    t = _relu_inputs(12, 3)
    out = run("clhip_relu_bwd", t, ("dy", "y", "dx"), (), 12)
    dx, dy = out["dx"], t["dy"]
    # +0.0, -0.0, NaN and negatives pass nothing (exact +0.0); the denormal and 2.0 pass dy bit for bit
    assert [int(v) for v in dx[:6].view(torch.int32)] == [0, 0, int(dy[2:3].view(torch.int32)), 0, 0, int(dy[5:6].view(torch.int32))]


# --------------------------------------------------------------------------- sigmoid
def sigmoid_x(n):
    head = torch.tensor([100.0, -100.0, 88.7, -88.7, 88.8, -88.8, 0.0, -0.0, 103.9, -103.9])
    return torch.cat([head, torch.linspace(-30.0, 30.0, n - head.numel())])


@pytest.mark.parametrize("n", [1013, N_SCALAR_WRAP])
def test_sigmoid_fwd_bwd(request, n):
    case = request.node.name
    x = sigmoid_x(n)
    out = run("clhip_sigmoid_fwd", dict(x=x, y=torch.full((n,), float("nan"))), ("x", "y"), (), n, mis=("y",))
    assert bitwise_equal(out["x"], x)
    y = out["y"]
    assert bool(torch.isfinite(y).all()), "sigmoid produced inf / NaN where fp64 has none"
    assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0
    fp32_chain_check(case, "sigmoid", y, torch.sigmoid(x), torch.sigmoid(x.double()), LOSS_BASE)
    gen = torch.Generator().manual_seed(9)
    dy = torch.randn(n, generator=gen)
    y_in = torch.sigmoid(x)
    back = run("clhip_sigmoid_bwd", dict(dy=dy, y=y_in, dx=torch.full((n,), float("nan"))), ("dy", "y", "dx"), (), n, mis=("dy",))
    assert bool(torch.isfinite(back["dx"]).all())
    y64 = y_in.double()
    fp32_chain_check(case, "sigmoid backward", back["dx"], dy * y_in * (1 - y_in), dy.double() * y64 * (1 - y64), LOSS_BASE)


# --------------------------------------------------------------------------- Adadelta
ADA = dict(lr=1.0, rho=0.9, eps=1e-6)


def adadelta64(theta, grad, sq, acc, wd):
    lr, rho, eps, wd = (float(np.float32(v)) for v in (ADA["lr"], ADA["rho"], ADA["eps"], wd))
    th, g, s, a = theta.double(), grad.double(), sq.double(), acc.double()
    if wd != 0:
        g = g + wd * th
    s = s * rho + (1 - rho) * g * g
    delta = torch.sqrt(a + eps) / torch.sqrt(s + eps) * g
    a = a * rho + (1 - rho) * delta * delta
    return th - lr * delta, s, a


def adadelta32(theta, grad, sq, acc, wd, step):
    p = theta.clone().requires_grad_(True)
    opt = torch.optim.Adadelta([p], lr=ADA["lr"], rho=ADA["rho"], eps=ADA["eps"], weight_decay=wd)
    p.grad = grad.clone()
    if step > 0:
        opt.state[p] = dict(step=torch.tensor(float(step)), square_avg=sq.clone(), acc_delta=acc.clone())
    opt.step()
    st = opt.state[p]
    return p.detach(), st["square_avg"], st["acc_delta"]


@pytest.mark.parametrize("wd", [0.0, 5e-4], ids=["no-decay", "decay"])
@pytest.mark.parametrize("n", [5, 1023, N_SCALAR_WRAP])
def test_adadelta_three_steps(request, n, wd):
    """Three steps from zero state, each from the device's own previous state; torch.optim.Adadelta on the CPU as comparator."""
    case = request.node.name
    gen = torch.Generator().manual_seed(n % 1000 + 51)
    theta, sq, acc = torch.randn(n, generator=gen), torch.zeros(n), torch.zeros(n)
    for step in range(3):
        grad = 0.1 * torch.randn(n, generator=gen)
        out = run("clhip_adadelta_step", dict(theta=theta, grad=grad, sq=sq, acc=acc), ("theta", "grad", "sq", "acc"),
                  (ADA["lr"], ADA["rho"], ADA["eps"], wd), n, mis=("theta", "acc"))
        assert bitwise_equal(out["grad"], grad)
        r64 = adadelta64(theta, grad, sq, acc, wd)
        r32 = adadelta32(theta, grad, sq, acc, wd, step)
        for k, name in enumerate(("theta", "sq", "acc")):
            fp32_chain_check(case, "%s after step %d" % (name, step + 1), out[name], r32[k], r64[k], HAT_BASE)
        theta, sq, acc = out["theta"], out["sq"], out["acc"]


# --------------------------------------------------------------------------- MSE
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("n", [1, 1023, 1025, 5000])
def test_mse_mean(request, n, scale):
    case = request.node.name
    gen = torch.Generator().manual_seed(n + 61)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    want_loss = ((a.double() - b.double()) ** 2).sum() / n
    g = (torch.tensor(2.0) * torch.tensor(scale)) / torch.tensor(float(n))           # float32: fl(fl(2 * scale) / n)
    want_da = g * (a - b)                                                           # fl(g * fl(a - b))
    for with_da in (True, False):
        _lib, L = _L()
        A = Arena()
        ka, kb, kda, kl = A.add(a, True), A.add(b), A.add(n, True, fill=NAN_BITS), A.add(1, fill=NAN_BITS)
        A.upload(dev())
        _lib.check(L.clhip_mse_mean(A.ptr(ka), A.ptr(kb), n, scale, A.ptr(kda) if with_da else None, A.ptr(kl), _stream()), "clhip_mse_mean")
        torch.cuda.synchronize()
        A.download()
        assert A.gaps_untouched() and bitwise_equal(A.get(ka), a) and bitwise_equal(A.get(kb), b)
        ulps = ulp_distance(A.get(kl), want_loss.float().view(1))
        print("MEASURED|%s|loss ulp from the rounded fp64 mean (da %s)|%d|2" % (case, "written" if with_da else "NULL", ulps))
        assert ulps <= 2, "loss %r, fp64 %r" % (float(A.get(kl)), float(want_loss))
        if with_da:
            d = ulp_distance(A.get(kda), want_da)
            print("MEASURED|%s|da ulp from fl(fl(2 * scale / n) * fl(a - b))|%d|0" % (case, d))
            assert d == 0 and bitwise_equal(A.get(kda), want_da)
        else:
            assert bool((A.get(kda).view(torch.int32) == NAN_BITS).all()), "da == NULL, yet something was written"


# --------------------------------------------------------------------------- IMM merge
@pytest.mark.parametrize("mode", ["mean", "mode"])
@pytest.mark.parametrize("n_models", [1, 2, 7, 32])
def test_imm_merge_bitwise(n_models, mode):
    _lib, L = _L()
    for n in (5, 4099):
        gen = torch.Generator().manual_seed(100 * n_models + n % 100)
        thetas = [torch.randn(n, generator=gen) for _ in range(n_models)]
        precs = [torch.rand(n, generator=gen) + 1e-3 for _ in range(n_models)]
        sum_prec = torch.zeros(n)
        for p in precs:
            sum_prec = sum_prec + p
        A = Arena()
        kt = [A.add(t, m % 2 == 1) for m, t in enumerate(thetas)]
        kp = [A.add(p, m % 3 == 1) for m, p in enumerate(precs)]
        ks, ko = A.add(sum_prec), A.add(n, True, fill=NAN_BITS)
        A.upload(dev())
        tp = (C.c_void_p * n_models)(*[A.ptr(k) for k in kt])
        pp = (C.c_void_p * n_models)(*[A.ptr(k) for k in kp])
        if mode == "mean":
            rc = L.clhip_imm_merge(tp, None, None, n_models, n, A.ptr(ko), _stream())
        else:
            rc = L.clhip_imm_merge(tp, pp, A.ptr(ks), n_models, n, A.ptr(ko), _stream())
        _lib.check(rc, "clhip_imm_merge")
        torch.cuda.synchronize()
        A.download()
        assert A.gaps_untouched()
        acc = torch.zeros(n)                                     # the float32 torch sequence: running sum from zero
        if mode == "mean":
            for t in thetas:
                acc = acc + t
            acc = acc / n_models                                  # divide last
        else:
            for t, p in zip(thetas, precs):
                acc = acc + (p / sum_prec) * t                    # div, mul, add as separate float32 operations
        got = A.get(ko)
        assert bitwise_equal(got, acc), "%s-IMM of %d models, n = %d: %d elements differ by up to %d ulp" % (
            mode, n_models, n, int((got.view(torch.int32) != acc.view(torch.int32)).sum()), ulp_distance(got, acc))
