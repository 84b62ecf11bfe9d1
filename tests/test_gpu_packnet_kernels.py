"""Kernel-level parity of csrc/packnet.hip.  Everything but the SGD arithmetic is exact: masks and zeroed weights bitwise, the
radix select `==` on the cutoff's bit pattern against torch.kthvalue(|w[mask == cur]|, k) on the CPU (cross-checked with
np.partition).

kth_abs: one candidate; a tie of 400 equal magnitudes (both signs) across ranks 301..700 asked at both of its edges; all
candidates equal; k = the candidate count; +-0.0, the smallest denormal, FLT_MIN, inf and one NaN among the candidates with k
walking through each; n = 2 * 2048 * 256 + 77 under a three-valued mask (the capped grid wraps); all calls of a case share one
workspace that starts as garbage (stale state).  `cur` absent from the mask and k one past the candidate count: the call
returns 0 and the status word (ws word 260) reads 1; the cutoff is not asserted, the wrapper refuses these inputs beforehand.
prune: ties at the cutoff go (<=), cutoffs 0.0 / denormal / NaN, -0.0 under masks 0 and cur becomes +0.0, foreign tasks'
weights and masks keep their bits.  Masks sit at odd byte offsets in an arena with sentinel gaps, weights one float past a
16-byte boundary.  packnet_sgd_step follows the fp32-chain rule (base 1e-6) against an fp64 restatement with
oracle.packnet_ref as the float32 comparator; grad and the zero pattern of theta are bitwise.

Measured on one MI355X (every figure is printed as `MEASURED|...` before it is asserted, run with -s):
  packnet_sgd_step (8 cases, worst over the sizes): theta                          5.9e-08 / 6.1e-08
  packnet_sgd_step: buf                                                            8.2e-08 / 8.2e-08
(device distance / float32 CPU distance from fp64, relative to the tensor's largest entry; everything else is exact.)
"""
import numpy as np
import pytest
import torch

from kernel_parity import HAT_BASE, Arena, ByteArena, bitwise_equal, fp32_chain_check
from oracle import packnet_ref as P

pytestmark = pytest.mark.gpu

WRAP = 2048 * 256
NAN_BITS = 0x7fc00000
DEN = float(np.frombuffer(np.uint32(1).tobytes(), dtype=np.float32)[0])        # the smallest positive denormal
FLT_MIN = float(np.finfo(np.float32).tiny)
STATUS_WORD = 260


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from clsurvey_amd import _lib
    return _lib, _lib.lib()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# --------------------------------------------------------------------------- kth_abs
class Kth:
    """w and mask uploaded once; every call shares one workspace, which starts as garbage."""

    def __init__(self, w, mask, mis=True):
        _lib, L = _L()
        self.w, self.mask = w, mask
        self.fa, self.ba = Arena(), ByteArena()
        self.kw = self.fa.add(w, mis)
        self.kout = self.fa.add(1, fill=NAN_BITS)
        self.km = self.ba.add(mask)
        self.fa.upload(dev())
        self.ba.upload(dev())
        self.ws = torch.full((L.clhip_packnet_kth_ws() // 4 + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev())

    def call(self, cur, k):
        """Returns (bit pattern of the cutoff, status word)."""
        _lib, L = _L()
        rc = L.clhip_packnet_kth_abs(self.fa.ptr(self.kw), self.ba.ptr(self.km), self.w.numel(), cur, k, self.fa.ptr(self.kout),
                                     self.ws.data_ptr(), L.clhip_packnet_kth_ws(), _stream())
        assert rc == 0, "clhip_packnet_kth_abs returned %d" % rc
        torch.cuda.synchronize()
        self.fa.download()
        self.ba.download()
        assert self.fa.gaps_untouched() and self.ba.gaps_untouched(), "kth_abs wrote outside its tensors"
        assert bitwise_equal(self.fa.get(self.kw), self.w) and torch.equal(self.ba.get(self.km), self.mask), "kth_abs modified its inputs"
        ws = self.ws.cpu()
        assert bool((ws[STATUS_WORD + 1:] == 0x5A5A5A5A).all()), "kth_abs wrote past its workspace"
        return int(bits(self.fa.get(self.kout))[0]), int(ws[STATUS_WORD])

    def check(self, cur, k):
        cand = self.w[self.mask == cur].abs()
        assert 1 <= k <= cand.numel()
        want = torch.kthvalue(cand, k).values.view(1)
        part = np.partition(cand.numpy(), k - 1)[k - 1:k]
        assert bits(want).tolist() == bits(torch.from_numpy(part.copy())).tolist(), "kthvalue and np.partition disagree"
        got, status = self.call(cur, k)
        assert status == 0, "status %d for rank %d of %d candidates" % (status, k, cand.numel())
        assert got == int(bits(want)[0]), "rank %d of %d: cutoff bits %#010x, torch.kthvalue %#010x (%r)" % (
            k, cand.numel(), got, int(bits(want)[0]), float(want))


def test_kth_abs_single_candidate():
    Kth(torch.tensor([-0.375]), torch.tensor([3], dtype=torch.uint8)).check(3, 1)
    # one candidate among foreign weights that are smaller and larger
    w = torch.tensor([1e-3, 5.0, -0.25, 7.0, 1e-6])
    Kth(w, torch.tensor([1, 1, 2, 0, 0], dtype=torch.uint8)).check(2, 1)


def test_kth_abs_tie_spanning_the_rank():
    gen = torch.Generator().manual_seed(3)
    small = 0.4 * torch.rand(300, generator=gen)                   # ranks 1..300, all < 0.5
    tie = torch.full((400,), 0.5)                                  # ranks 301..700
    tie[::2] = -0.5
    large = 0.6 + torch.rand(300, generator=gen)                   # ranks 701..1000
    w = torch.cat([small, tie, large])[torch.randperm(1000, generator=gen)]
    w = w * torch.where(torch.rand(1000, generator=gen) < 0.5, -1.0, 1.0)
    kth = Kth(w, torch.full((1000,), 2, dtype=torch.uint8))
    for k in (300, 301, 500, 700, 701):
        kth.check(2, k)
    srt = w.abs().sort().values
    assert float(srt[299]) < 0.5 == float(srt[300]) == float(srt[699]) < float(srt[700])


def test_kth_abs_all_equal_and_k_at_the_count():
    w = torch.full((257,), 0.75)
    w[1::3] = -0.75
    mask = torch.full((257,), 1, dtype=torch.uint8)
    kth = Kth(w, mask)
    for k in (1, 128, 257):
        kth.check(1, k)
    gen = torch.Generator().manual_seed(4)
    w = torch.randn(1023, generator=gen)
    mask = torch.randint(0, 3, (1023,), generator=gen).to(torch.uint8)
    kth = Kth(w, mask)
    count = int((mask == 1).sum())
    for k in (count, 1, count - 1, count):                        # the same workspace, ranks up and down
        kth.check(1, k)


def test_kth_abs_zeros_denormals_inf_nan():
    w = torch.tensor([0.5, float("nan"), -0.0, -FLT_MIN, DEN, float("-inf"), 0.0, -2.0, 3e-39])
    mask = torch.full((w.numel(),), 4, dtype=torch.uint8)
    kth = Kth(w, mask)
    for k in range(1, w.numel() + 1):                              # 0, 0, denormal, 3e-39, FLT_MIN, 0.5, 2, inf, NaN
        kth.check(4, k)
    got = [kth.call(4, k)[0] for k in (1, 2, 3, 8, 9)]                # by hand: +0.0 twice, the denormal, inf, NaN
    assert got == [0, 0, 1, 0x7f800000, NAN_BITS], [hex(g) for g in got]


def test_kth_abs_grid_wraps():
    n = 2 * WRAP + 77
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(n, generator=gen) * 0.05
    w[::1000] = 0.0
    mask = torch.randint(0, 3, (n,), generator=gen).to(torch.uint8)
    mask[-77:] = 2                                                 # the tail past the last full stride belongs to `cur`
    w[-1] = 9.0                                                    # and holds the largest candidate
    kth = Kth(w, mask)
    count = int((mask == 2).sum())
    for k in (1, count // 2, count):
        kth.check(2, k)


def test_kth_abs_out_of_range_sets_the_status_word():
    gen = torch.Generator().manual_seed(6)
    w = torch.randn(300, generator=gen)
    mask = torch.randint(0, 3, (300,), generator=gen).to(torch.uint8)
    kth = Kth(w, mask)
    count = int((mask == 1).sum())
    kth.check(1, count)                                            # in range: status 0
    assert kth.call(1, count + 1)[1] == 1, "k one past the candidate count must set the status word"
    kth.check(1, 1)                                                # and the next call clears it
    assert kth.call(7, 1)[1] == 1, "`cur` absent from the mask must set the status word"
    kth.check(2, 5)


# --------------------------------------------------------------------------- prune and the mask kernels
def special_weights(n, gen):
    pool = torch.tensor([0.0, -0.0, DEN, -DEN, 2 * DEN, -FLT_MIN, 0.25, -0.25, 0.5, -0.5, 0.5, 1.0, float("inf"), float("nan")])
    w = pool[torch.randint(0, pool.numel(), (n,), generator=gen)]
    r = torch.randn(n, generator=gen)
    return torch.where(torch.rand(n, generator=gen) < 0.4, r, w)


def masks_of(n, gen, values):
    v = torch.tensor(values, dtype=torch.uint8)
    return v[torch.randint(0, v.numel(), (n,), generator=gen)] if n >= len(values) else v[:n].clone()


def run_masked(fn_name, w, mask, args_after, mis=True, extra_float=None):
    """Calls L.<fn_name>(w, mask, n, *args_after, stream) with w in a float arena and mask in a byte arena; extra_float: one
    more float tensor whose pointer is appended after `cur` (prune's cutoff).  Returns w, mask after the call."""
    _lib, L = _L()
    fa, ba = Arena(), ByteArena()
    kw = fa.add(w, mis)
    kx = fa.add(extra_float) if extra_float is not None else None
    km = ba.add(mask)
    fa.upload(dev())
    ba.upload(dev())
    assert ba.ptr(km) % 2 == 1
    args = list(args_after) + ([fa.ptr(kx)] if kx is not None else [])
    _lib.check(getattr(L, fn_name)(fa.ptr(kw), ba.ptr(km), w.numel(), *args, _stream()), fn_name)
    torch.cuda.synchronize()
    fa.download()
    ba.download()
    assert fa.gaps_untouched() and ba.gaps_untouched(), fn_name + " wrote outside its tensors"
    if kx is not None:
        assert bitwise_equal(fa.get(kx), extra_float.reshape(-1))
    return fa.get(kw).clone(), ba.get(km).clone()


PRUNE_N = [1, 255, 257, WRAP + 3]


@pytest.mark.parametrize("cut", [0.5, 0.0, DEN, float("nan")], ids=["tie", "zero", "denormal", "nan"])
@pytest.mark.parametrize("n", PRUNE_N)
def test_prune(n, cut):
    cur = 2
    gen = torch.Generator().manual_seed(n % 1000 + 11)
    w = special_weights(n, gen)
    mask = masks_of(n, gen, [2, 0, 1, 3, 2, 255])
    if n == 1:
        w = torch.tensor([-0.5 if cut == 0.5 else -0.0])
    else:                                                          # by hand: -0.0 under masks 0 and cur, ties of both owners
        w[3:10] = torch.tensor([-0.0, -0.0, float("nan"), 0.5, -0.5, DEN, -0.5])
        mask[3:10] = torch.tensor([0, cur, 0, cur, 3, cur, cur], dtype=torch.uint8)
    cutoff = torch.tensor([cut], dtype=torch.float32)
    w2, m2 = run_masked("clhip_packnet_prune", w, mask, (cur,), extra_float=cutoff)
    go = (mask == cur) & (w.abs() <= cutoff)                       # ties go; NaN compares false: nothing goes
    want_m = torch.where(go, torch.zeros_like(mask), mask)
    want_w = torch.where(want_m == 0, torch.zeros_like(w), w)      # +0.0, whatever was there (-0.0, NaN, inf)
    if n > 1:
        assert bool(go.any()) != (cut != cut), "the cutoff must release something unless it is NaN"
    if n >= 255:
        assert bool((bits(w)[(mask == 0) | go] == -(1 << 31)).any()), "no -0.0 among the released weights"
    assert torch.equal(m2, want_m), "%d mask bytes differ" % int((m2 != want_m).sum())
    assert bitwise_equal(w2, want_w), "%d weights differ" % int((bits(w2) != bits(want_w)).sum())
    foreign = (mask != 0) & (mask != cur)
    assert torch.equal(m2[foreign], mask[foreign]) and torch.equal(bits(w2)[foreign], bits(w)[foreign]), "a foreign task's weight moved"
    assert bool((bits(w2)[want_m == 0] == 0).all())


@pytest.mark.parametrize("n", PRUNE_N)
def test_finetune_mask_and_mask_grad_zero(n):
    _lib, L = _L()
    gen = torch.Generator().manual_seed(n % 1000 + 21)
    g = special_weights(n, gen)
    mask = masks_of(n, gen, [0, 1, 2, 3, 0, 254])
    # finetune_mask has no float tensor: the byte arena alone
    ba = ByteArena()
    km = ba.add(mask)
    ba.upload(dev())
    _lib.check(L.clhip_packnet_finetune_mask(ba.ptr(km), n, 3, _stream()), "clhip_packnet_finetune_mask")
    torch.cuda.synchronize()
    ba.download()
    assert ba.gaps_untouched()
    assert torch.equal(ba.get(km), torch.from_numpy(P.make_finetuning_mask(mask.numpy(), 3)))
    g2, m2 = run_masked("clhip_mask_grad_zero", g, mask, (2,))
    assert torch.equal(m2, mask)
    assert bitwise_equal(g2, torch.where(mask != 2, torch.zeros_like(g), g))


@pytest.mark.parametrize("n", PRUNE_N)
def test_mask_weight_zero(n):
    gen = torch.Generator().manual_seed(n % 1000 + 31)
    w = special_weights(n, gen)
    mask = masks_of(n, gen, [0, 1, 2, 3, 4])
    w2, m2 = run_masked("clhip_mask_weight_zero", w, mask, (0, 0))
    assert torch.equal(m2, mask) and bitwise_equal(w2, torch.where(mask == 0, torch.zeros_like(w), w)), "mode 0"
    w3, _ = run_masked("clhip_mask_weight_zero", w, mask, (0, 3))       # mode 0 ignores idx
    assert bitwise_equal(w3, w2)
    for idx in range(5):
        w2, m2 = run_masked("clhip_mask_weight_zero", w, mask, (1, idx))
        want = torch.where((mask == 0) | (mask > idx), torch.zeros_like(w), w)
        assert torch.equal(m2, mask) and bitwise_equal(w2, want), "mode 1, idx %d: %d weights differ" % (idx, int((bits(w2) != bits(want)).sum()))


# --------------------------------------------------------------------------- packnet_sgd_step
LR, MOMENTUM = 0.05, 0.9
SGD_N = [1, 5, 255, 257, 1023, WRAP + 3]


def sgd64(theta, grad, buf, mask, cur, lr, momentum, wd, first):
    """The kernel's formula in fp64 on the float32 inputs (constants rounded to float32 as the entry point receives them)."""
    lr, momentum, wd = (float(np.float32(v)) for v in (lr, momentum, wd))
    th, g = theta.double(), grad.double()
    if mask is not None:
        g = torch.where(mask != cur, torch.zeros_like(g), g)
    d = g + (wd * th) * (g != 0).double() if wd != 0 else g
    b = d if first else buf.double() * momentum + d
    th = th - lr * b
    if mask is not None:
        th = torch.where(mask == 0, torch.zeros_like(th), th)
    return th, g, b


def sgd32(theta, grad, buf, mask, cur, lr, momentum, wd, first):
    g = P.make_grads_zero(grad.numpy(), mask.numpy(), cur) if mask is not None else grad.numpy().copy()
    th, b = P.packnet_sgd_step(theta.numpy(), g, None if first else buf.numpy(), lr, momentum, wd, first)
    if mask is not None:
        th = P.make_pruned_zero(th, mask.numpy())
    return torch.from_numpy(th), torch.from_numpy(g), torch.from_numpy(b)


@pytest.mark.parametrize("wd", [5e-4, 0.0], ids=["decay", "no-decay"])
@pytest.mark.parametrize("first", [1, 0], ids=["first", "later"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "no-mask"])
def test_packnet_sgd_step(request, with_mask, first, wd):
    _lib, L = _L()
    case = request.node.name
    cur = 2
    for n in SGD_N:
        gen = torch.Generator().manual_seed(n % 1000 + 41)
        theta = torch.randn(n, generator=gen) * 0.1
        grad = torch.randn(n, generator=gen)
        grad[torch.rand(n, generator=gen) < 0.25] = 0.0                 # exactly 0: no decay there
        if n >= 5:
            grad[1], grad[3] = 0.0, -0.0
        buf = torch.randn(n, generator=gen) * 0.01
        mask = masks_of(n, gen, [2, 0, 1, 255, 2]) if with_mask else None
        fa, ba = Arena(), ByteArena()
        kt, kg, kb = fa.add(theta, True), fa.add(grad), fa.add(buf, True)
        km = ba.add(mask) if with_mask else None
        fa.upload(dev())
        ba.upload(dev())
        _lib.check(L.clhip_packnet_sgd_step(fa.ptr(kt), fa.ptr(kg), fa.ptr(kb), ba.ptr(km) if with_mask else None, n, cur, LR, MOMENTUM, wd,
                                            first, _stream()), "clhip_packnet_sgd_step")
        torch.cuda.synchronize()
        fa.download()
        ba.download()
        assert fa.gaps_untouched() and ba.gaps_untouched(), "the step wrote outside its tensors"
        if with_mask:
            assert torch.equal(ba.get(km), mask), "the step changed the mask"
        th1, g1, b1 = fa.get(kt), fa.get(kg), fa.get(kb)
        r64 = sgd64(theta, grad, buf, mask, cur, LR, MOMENTUM, wd, first)
        r32 = sgd32(theta, grad, buf, mask, cur, LR, MOMENTUM, wd, first)
        want_g = torch.where(mask != cur, torch.zeros_like(grad), grad) if with_mask else grad
        assert bitwise_equal(g1, want_g), "n = %d: grad is not the masked gradient bit for bit" % n
        assert bitwise_equal(r32[1], want_g)
        fp32_chain_check(case, "theta n = %d" % n, th1, r32[0], r64[0], HAT_BASE)
        fp32_chain_check(case, "buf n = %d" % n, b1, r32[2], r64[2], HAT_BASE)
        assert torch.equal(th1 == 0, r32[0] == 0), "n = %d: the zero pattern of theta differs from the reference's" % n
        if with_mask:
            assert bool((bits(th1)[mask == 0] == 0).all()), "a pruned weight is not +0.0"
            if n >= 255:
                assert bool(((mask == 255) & (grad != 0)).any()) and bool(((mask == cur) & (grad == 0)).any())
