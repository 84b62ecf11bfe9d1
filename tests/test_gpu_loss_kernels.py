"""Kernel-level parity of csrc/loss.hip: every dispatch path of clhip_softmax_ce_slice, clhip_lwf_loss, clhip_mse_zero_sum
and the wide branch of clhip_loss_segments, each against the same formula in fp64 on the CPU from the same float32 inputs.

Which kernel a (N, ld, col_off, ncols) problem reaches — from the three conditions of clhip_softmax_ce_slice, in order:
  1. ncols <= 64 and N <= 1024 and N * (ld | 1) <= 12288   -> softmax_ce_rows_lds_kernel  ("lds")
  2. ncols <= 64 and N <= 1024 and ld <= 4096              -> softmax_ce_rows_kernel      ("rows")
  3. otherwise softmax_ce_kernel<16>, whose branch is `narrow` when ncols <= 64            ("narrow" / "wide")

  shape (N, ld, col_off, ncols)   kernel   why
  (1, 1, 0, 1)                    lds      1 * 1 = 1 <= 12288
  (7, 20, 0, 20)                  lds      7 * 21 = 147
  (200, 45, 20, 20)               lds      200 * 45 = 9000
  (64, 64, 0, 64)                 lds      64 * 65 = 4160, ncols = 64 is still "<= 64"
  (1000, 20, 0, 20)               rows     1000 * 21 = 21000 > 12288; N <= 1024, ld <= 4096
  (1024, 33, 5, 17)               rows     1024 * 33 = 33792 > 12288; N = 1024 is still "<= 1024"
  (300, 70, 3, 64)                rows     300 * 71 = 21300 > 12288
  (1025, 20, 0, 20)               narrow   N > 1024 fails 1 and 2; ncols <= 64
  (1500, 40, 20, 20)              narrow   N > 1024
  (3, 4100, 4000, 64)             narrow   3 * 4101 = 12303 > 12288 fails 1, ld > 4096 fails 2; ncols <= 64
  (5, 65, 0, 65)                  wide     ncols > 64 fails 1 and 2
  (33, 150, 0, 150)               wide     ncols > 64
  (17, 300, 100, 129)             wide     ncols > 64 (three column rounds of the 64 lanes, the last one a single lane)
  (200, 1000, 0, 1000)            wide     ncols > 64
expected_path() below restates the three conditions and every case asserts that its row of the table agrees with them.

Tolerances (kernel_parity.fp32_chain_check): distance from fp64 relative to the tensor's largest entry
<= max(1e-5, 4 x float32 CPU distance).  Counts, zeros outside a slice and the statistics' accumulation are exact.

Measured on one MI355X (worst over the checks of a case: device distance / float32-CPU distance from fp64, both
relative to the tensor's largest entry; every check prints a `MEASURED|...` line before it asserts, run with -s):
  softmax_ce_slice_every_path[lds-1x1x0x1]                                       0.0e+00 / 0.0e+00
  softmax_ce_slice_every_path[lds-7x20x0x20]                                     3.3e-07 / 1.3e-07
  softmax_ce_slice_every_path[lds-200x45x20x20]                                  3.2e-07 / 2.0e-07
  softmax_ce_slice_every_path[lds-64x64x0x64]                                    1.4e-07 / 1.2e-07
  softmax_ce_slice_every_path[rows-1000x20x0x20]                                 3.1e-07 / 2.4e-07
  softmax_ce_slice_every_path[rows-1024x33x5x17]                                 2.9e-07 / 2.7e-07
  softmax_ce_slice_every_path[rows-300x70x3x64]                                  3.8e-07 / 1.6e-07
  softmax_ce_slice_every_path[narrow-1025x20x0x20]                               2.1e-07 / 2.3e-07
  softmax_ce_slice_every_path[narrow-1500x40x20x20]                              2.1e-07 / 2.4e-07
  softmax_ce_slice_every_path[narrow-3x4100x4000x64]                             8.9e-08 / 8.4e-08
  softmax_ce_slice_every_path[wide-5x65x0x65]                                    7.2e-08 / 8.5e-08
  softmax_ce_slice_every_path[wide-33x150x0x150]                                 8.2e-08 / 1.1e-07
  softmax_ce_slice_every_path[wide-17x300x100x129]                               1.3e-07 / 7.9e-08
  softmax_ce_slice_every_path[wide-200x1000x0x1000]                              3.3e-07 / 3.3e-07
  softmax_ce_slice_scale_30_and_minus_inf[lds-200x45x20x20]                      1.6e-07 / 1.6e-07
  softmax_ce_slice_scale_30_and_minus_inf[rows-1024x33x5x17]                     1.6e-07 / 2.0e-07
  softmax_ce_slice_scale_30_and_minus_inf[narrow-1500x40x20x20]                  1.8e-07 / 2.5e-07
  softmax_ce_slice_scale_30_and_minus_inf[wide-17x300x100x129]                   1.5e-07 / 1.9e-07
  row-independence                                                               3.4e-07 / 2.5e-07
  lwf_loss_against_fp64[1-one-T1-lam0.5-d1-tp0-zp0]                              6.2e-08 / 2.0e-08
  lwf_loss_against_fp64[37-one-T2-lam10-d0-tp0-zp3]                              1.1e-07 / 9.6e-08
  lwf_loss_against_fp64[1024-one-T4-lam0.5-d1-tp0-zp3]                           1.9e-07 / 1.6e-07
  lwf_loss_against_fp64[1-two-T2-lam10-d1-tp0-zp3]                               7.7e-08 / 6.3e-08
  lwf_loss_against_fp64[37-two-T1-lam0.5-d1-tp2-zp0]                             1.5e-07 / 1.5e-07
  lwf_loss_against_fp64[1024-two-T4-lam10-d0-tp0-zp3]                            5.8e-07 / 1.7e-07
  lwf_loss_against_fp64[1-four-T4-lam0.5-d1-tp5-zp3]                             7.3e-08 / 7.3e-08
  lwf_loss_against_fp64[37-four-T2-lam10-d1-tp0-zp3]                             2.8e-07 / 2.6e-07
  lwf_loss_against_fp64[1024-four-T1-lam0.5-d1-tp5-zp0]                          2.3e-07 / 2.3e-07
  lwf_loss_against_fp64[1-many-T1-lam10-d1-tp0-zp0]                              8.9e-08 / 1.4e-07
  lwf_loss_against_fp64[37-many-T4-lam0.5-d1-tp4-zp3]                            1.4e-07 / 1.4e-07
  lwf_loss_against_fp64[1024-many-T2-lam10-d1-tp0-zp3]                           2.8e-07 / 3.1e-07
  lwf_loss_against_fp64[37-many-T2-lam10-d0-tp4-zp3]                             1.4e-07 / 1.4e-07
  mse_zero_sum_against_fp64[1]                                                   2.0e-08 / 2.0e-08
  mse_zero_sum_against_fp64[63]                                                  1.7e-08 / 1.7e-08
  mse_zero_sum_against_fp64[1024]                                                5.0e-08 / 5.0e-08
  mse_zero_sum_against_fp64[1025]                                                1.2e-08 / 1.2e-07
  mse_zero_sum_against_fp64[30000]                                               8.7e-09 / 1.1e-07
  loss_segments_wide_slices                                                      2.5e-07 / 1.8e-07
  row-independence: ulp distance lds vs rows                                     0
"""
import ctypes as C

import pytest
import torch

from kernel_parity import LOSS_BASE, bitwise_equal, fp32_chain_check, ulp_distance
from oracle import lwf_ref

pytestmark = pytest.mark.gpu

OUTSIDE = 1.0e4          # logits outside the slice / past the heads: larger than anything inside, so a leak shows at once


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def expected_path(N, ld, ncols):
    if ncols <= 64 and N <= 1024 and N * (ld | 1) <= 12288:
        return "lds"
    if ncols <= 64 and N <= 1024 and ld <= 4096:
        return "rows"
    return "narrow" if ncols <= 64 else "wide"


CE_SHAPES = [
    ("lds", (1, 1, 0, 1)), ("lds", (7, 20, 0, 20)), ("lds", (200, 45, 20, 20)), ("lds", (64, 64, 0, 64)),
    ("rows", (1000, 20, 0, 20)), ("rows", (1024, 33, 5, 17)), ("rows", (300, 70, 3, 64)),
    ("narrow", (1025, 20, 0, 20)), ("narrow", (1500, 40, 20, 20)), ("narrow", (3, 4100, 4000, 64)),
    ("wide", (5, 65, 0, 65)), ("wide", (33, 150, 0, 150)), ("wide", (17, 300, 100, 129)), ("wide", (200, 1000, 0, 1000)),
]
# one shape per path for the scale-30 / -inf case and the tie rule (every one has a column offset and >= 3 columns)
ONE_PER_PATH = [("lds", (200, 45, 20, 20)), ("rows", (1024, 33, 5, 17)), ("narrow", (1500, 40, 20, 20)),
                ("wide", (17, 300, 100, 129))]


def _ids(cases):
    return ["%s-%s" % (p, "x".join(str(v) for v in s)) for p, s in cases]


def _problem(shape, scale, seed):
    N, ld, off, nc = shape
    gen = torch.Generator().manual_seed(seed)
    z = torch.full((N, ld), OUTSIDE)
    z[:, off:off + nc] = torch.randn((N, nc), generator=gen) * scale
    y = torch.randint(0, nc, (N,), generator=gen)
    return z, y


def lowest_index_hits(zs, y):
    """#rows whose label is the FIRST column attaining the row maximum (torch.max's rule), spelled out."""
    m = zs.max(1, keepdim=True).values
    idx = torch.arange(zs.shape[1]).expand_as(zs)
    first = torch.where(zs == m, idx, torch.full_like(idx, zs.shape[1])).min(1).values
    return int((first == y).sum())


def ce_reference(z, y, shape, reduction, dtype):
    """Loss and the full [N][ld] gradient (zero outside the slice) of the sliced softmax cross-entropy, written out."""
    N, ld, off, nc = shape
    zs = z[:, off:off + nc].to(dtype)
    m = zs.max(1, keepdim=True).values
    ex = torch.exp(zs - m)
    lse = torch.log(ex.sum(1, keepdim=True))
    logp = zs - m - lse
    rows = torch.arange(N)
    loss = -logp[rows, y].sum()
    onehot = torch.zeros_like(zs)
    onehot[rows, y] = 1
    g = torch.exp(logp) - onehot
    if reduction == 0:
        loss, g = loss / N, g / N
    full = torch.zeros((N, ld), dtype=dtype)
    full[:, off:off + nc] = g
    return loss.reshape(1), full


def run_ce(z, y, shape, reduction, stats=None):
    from clsurvey_amd import _lib
    N, ld, off, nc = shape
    d = dev()
    zd, yd = z.to(d), y.to(d)
    dz = torch.full((N, ld), float("nan"), device=d)                 # sentinel: an unwritten element stays NaN
    loss = torch.full((1,), float("nan"), device=d)
    _lib.check(_lib.lib().clhip_softmax_ce_slice(zd.data_ptr(), yd.data_ptr(), N, ld, off, nc, reduction, dz.data_ptr(),
                                                 loss.data_ptr(), stats.data_ptr() if stats is not None else None, _stream()),
               "clhip_softmax_ce_slice")
    torch.cuda.synchronize()
    return loss.cpu(), dz.cpu()


def check_ce(case, path, shape, z, y):
    N, ld, off, nc = shape
    assert expected_path(N, ld, nc) == path, "the dispatch table of this file disagrees with clhip_softmax_ce_slice's conditions"
    hits = lowest_index_hits(z[:, off:off + nc], y)
    outside = torch.ones(ld, dtype=torch.bool)
    outside[off:off + nc] = False
    for reduction, name in ((0, "mean"), (1, "sum")):
        stats = torch.zeros(2, dtype=torch.float64, device=dev())
        loss, dz = run_ce(z, y, shape, reduction, stats)
        loss_b, dz_b = run_ce(z, y, shape, reduction, stats)
        l32, g32 = ce_reference(z, y, shape, reduction, torch.float32)
        l64, g64 = ce_reference(z, y, shape, reduction, torch.float64)
        fp32_chain_check(case, "loss " + name, loss, l32, l64, LOSS_BASE)
        fp32_chain_check(case, "dlogits " + name, dz, g32, g64, LOSS_BASE)
        assert bool((dz[:, outside] == 0).all()), "dlogits outside the slice must be exactly 0"
        assert bitwise_equal(loss, loss_b) and bitwise_equal(dz, dz_b), "one block, fixed order: two calls must agree bitwise"
        s = stats.cpu()
        assert float(s[0]) == 2.0 * float(loss[0]), "stats[0] must accumulate the float loss of both calls"
        assert float(s[1]) == 2.0 * hits, "stats[1]: %r, exact count %d per call" % (float(s[1]), hits)


@pytest.mark.parametrize("path,shape", CE_SHAPES, ids=_ids(CE_SHAPES))
def test_softmax_ce_slice_every_path(request, path, shape):
    z, y = _problem(shape, 3.0, 11)
    check_ce(request.node.name, path, shape, z, y)


@pytest.mark.parametrize("path,shape", ONE_PER_PATH, ids=_ids(ONE_PER_PATH))
def test_softmax_ce_slice_scale_30_and_minus_inf(request, path, shape):
    N, ld, off, nc = shape
    z, y = _problem(shape, 30.0, 12)
    r = N // 2
    z[r, off + (int(y[r]) + 1) % nc] = float("-inf")                 # a non-label column of one row
    check_ce(request.node.name, path, shape, z, y)


def tie_problem(path, shape, mode):
    """Logits whose first rows attain their maximum at two or three columns with identical float32 values; every tied row's
    label is the first, the second or the last of its tied columns (mode).  Returns z, y and the tied column tuples."""
    N, ld, off, nc = shape
    z, y = _problem(shape, 3.0, 13)
    gen = torch.Generator().manual_seed(14)
    ties = []
    if path == "wide":                                # columns 63 | 64 sit in lane 63 of the first round and lane 0 of the second;
        ties += [(63, 64), (5, 69), (0, 128), (63, 64, 128), (1, 65, 66)]       # c and c + 64 share a lane
    rows = min(N, 60)
    while len(ties) < rows:
        k = 2 + len(ties) % 2
        ties.append(tuple(sorted(torch.randperm(nc, generator=gen)[:k].tolist())))
    for r, cols in enumerate(ties):
        for c in cols:
            z[r, off + c] = 50.0
        y[r] = cols[{"first": 0, "second": 1, "last": -1}[mode]]
    return z, y, ties


@pytest.mark.parametrize("mode", ["first", "second", "last"])
@pytest.mark.parametrize("path,shape", ONE_PER_PATH, ids=_ids(ONE_PER_PATH))
def test_softmax_ce_tie_rule_lowest_index(path, shape, mode):
    """Only `label == first tied column` counts as correct (torch.max's lowest-index rule): with the label on the first tied
    column every tied row is a hit, with it on the second or the last one none is.  A last-index rule would count the other
    way round, an any-tied-column rule would count every tied row in all three modes."""
    N, ld, off, nc = shape
    assert expected_path(N, ld, nc) == path
    z, y, ties = tie_problem(path, shape, mode)
    rows = len(ties)
    zs = z[:, off:off + nc]
    hits = lowest_index_hits(zs, y)
    untied = lowest_index_hits(zs[rows:], y[rows:])
    assert rows > 0 and hits == untied + (rows if mode == "first" else 0)        # the rule, stated without any arg-max
    assert any(len(c) == 3 for c in ties) and (path != "wide" or (63, 64) in ties)
    stats = torch.zeros(2, dtype=torch.float64, device=dev())
    run_ce(z, y, shape, 1, stats)
    assert float(stats.cpu()[1]) == float(hits), "correct-count %r, lowest-index rule %d (%d tied rows, label on the %s tied column)" % (
        float(stats.cpu()[1]), hits, rows, mode)


def test_softmax_ce_rows_are_independent_of_the_path():
    """reduction = sum: the 200 rows of a (200, 20) problem (LDS kernel) are the first 200 rows of a (1000, 20) problem (rows
    kernel); the LDS kernel's header says the arithmetic is the same, so the 200 gradient rows are expected bitwise equal."""
    assert expected_path(200, 20, 20) == "lds" and expected_path(1000, 20, 20) == "rows"
    z, y = _problem((1000, 20, 0, 20), 3.0, 15)
    _, big = run_ce(z, y, (1000, 20, 0, 20), 1)
    _, small = run_ce(z[:200].contiguous(), y[:200].contiguous(), (200, 20, 0, 20), 1)
    ulps = ulp_distance(small, big[:200])
    print("MEASURED|row-independence|ulp distance lds vs rows|%d|0" % ulps)
    _, g32 = ce_reference(z, y, (1000, 20, 0, 20), 1, torch.float32)
    _, g64 = ce_reference(z, y, (1000, 20, 0, 20), 1, torch.float64)
    fp32_chain_check("row-independence", "dlogits rows kernel", big, g32, g64, LOSS_BASE)
    fp32_chain_check("row-independence", "dlogits lds kernel", small, g32[:200], g64[:200], LOSS_BASE)
    assert ulps == 0, "the two row kernels differ by up to %d ulp on the same rows" % ulps


# --------------------------------------------------------------------------- clhip_lwf_loss
HEADS = {"one": [5], "two": [3, 4], "four": [20, 20, 20, 7], "many": [(5 * i) % 9 + 1 for i in range(32)]}
LWF_CASES = [
    # N, layout, T, lam, distill, teacher columns past the old heads, logit columns past the heads
    (1, "one", 1.0, 0.5, 1, 0, 0), (37, "one", 2.0, 10.0, 0, 0, 3), (1024, "one", 4.0, 0.5, 1, 0, 3),
    (1, "two", 2.0, 10.0, 1, 0, 3), (37, "two", 1.0, 0.5, 1, 2, 0), (1024, "two", 4.0, 10.0, 0, 0, 3),
    (1, "four", 4.0, 0.5, 1, 5, 3), (37, "four", 2.0, 10.0, 1, 0, 3), (1024, "four", 1.0, 0.5, 1, 5, 0),
    (1, "many", 1.0, 10.0, 1, 0, 0), (37, "many", 4.0, 0.5, 1, 4, 3), (1024, "many", 2.0, 10.0, 1, 0, 3),
    (37, "many", 2.0, 10.0, 0, 4, 3),
]


def lwf_reference(z, y, teacher, sizes, T, lam, distill, dtype):
    z = z.detach().clone().to(dtype).requires_grad_(True)
    offs = [sum(sizes[:h]) for h in range(len(sizes))]
    heads = [z[:, o:o + c] for o, c in zip(offs, sizes)]
    if distill and len(sizes) > 1:
        tt = [teacher[:, o:o + c].to(dtype) for o, c in zip(offs[:-1], sizes[:-1])]
        task, dist = lwf_ref.lwf_objective(heads, y, tt, T, lam)
    else:
        task, dist = lwf_ref.lwf_objective(heads[-1:], y, [], T, lam)
        dist = torch.zeros((), dtype=dtype)
    (task + dist).backward()
    return torch.stack([task.detach(), dist.detach()]), z.grad


@pytest.mark.parametrize("N,layout,T,lam,distill,t_pad,z_pad", LWF_CASES,
                         ids=["%d-%s-T%g-lam%g-d%d-tp%d-zp%d" % c for c in LWF_CASES])
def test_lwf_loss_against_fp64(request, N, layout, T, lam, distill, t_pad, z_pad):
    from clsurvey_amd import _lib
    case = request.node.name
    sizes = HEADS[layout]
    assert len(sizes) <= 32 and min(sizes) >= 1 and sizes[-1] > 1
    width, old = sum(sizes), sum(sizes[:-1])
    ld, ld_t = width + z_pad, old + t_pad
    gen = torch.Generator().manual_seed(21)
    z = torch.full((N, ld), OUTSIDE)
    z[:, :width] = torch.randn((N, width), generator=gen) * 3
    y = torch.randint(0, sizes[-1], (N,), generator=gen)
    teacher = None
    if len(sizes) > 1:                                # a single head has nothing to distil: teacher stays NULL
        teacher = torch.full((N, ld_t), OUTSIDE)
        teacher[:, :old] = torch.randn((N, old), generator=gen) * 3
    d = dev()
    zd, yd = z.to(d), y.to(d)
    td = teacher.to(d) if teacher is not None else None
    dz = torch.full((N, ld), float("nan"), device=d)
    loss2 = torch.full((2,), float("nan"), device=d)
    seed_stats = [1.5, 3.0]
    stats = torch.tensor(seed_stats, dtype=torch.float64, device=d)
    hs = (C.c_int * len(sizes))(*sizes)
    _lib.check(_lib.lib().clhip_lwf_loss(zd.data_ptr(), yd.data_ptr(), td.data_ptr() if td is not None else None, hs, len(sizes), N,
                                         ld, ld_t, T, lam, distill, dz.data_ptr(), loss2.data_ptr(), stats.data_ptr(), _stream()),
               "clhip_lwf_loss")
    torch.cuda.synchronize()
    loss2, dz, stats = loss2.cpu(), dz.cpu(), stats.cpu()
    l32, g32 = lwf_reference(z, y, teacher, sizes, T, lam, distill, torch.float32)
    l64, g64 = lwf_reference(z, y, teacher, sizes, T, lam, distill, torch.float64)
    fp32_chain_check(case, "task loss", loss2[0:1], l32[0:1], l64[0:1], LOSS_BASE)
    if distill and len(sizes) > 1:
        fp32_chain_check(case, "lambda * distillation", loss2[1:2], l32[1:2], l64[1:2], LOSS_BASE)
    else:
        assert float(loss2[1]) == 0.0
    fp32_chain_check(case, "dlogits", dz, g32, g64, LOSS_BASE)
    assert bool((dz[:, width:] == 0).all()), "dlogits past the last head must be exactly 0"
    if not distill:
        assert bool((dz[:, :old] == 0).all()), "distill = 0: no gradient on the old heads"
    assert float(stats[0]) == seed_stats[0] + float(loss2[0])
    assert float(stats[1]) == seed_stats[1] + lowest_index_hits(z[:, old:width], y)


# --------------------------------------------------------------------------- clhip_mse_zero_sum
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 200 * 150])
def test_mse_zero_sum_against_fp64(request, n):
    from clsurvey_amd import _lib
    z = torch.randn(n, generator=torch.Generator().manual_seed(31)) * 3
    d = dev()
    zd = z.to(d)
    dz = torch.full((n,), float("nan"), device=d)
    loss = torch.full((1,), float("nan"), device=d)
    _lib.check(_lib.lib().clhip_mse_zero_sum(zd.data_ptr(), n, dz.data_ptr(), loss.data_ptr(), _stream()), "clhip_mse_zero_sum")
    torch.cuda.synchronize()
    fp32_chain_check(request.node.name, "loss", loss, (z * z).sum().reshape(1), (z.double() ** 2).sum().reshape(1), LOSS_BASE)
    fp32_chain_check(request.node.name, "dz", dz, 2 * z, 2 * z.double(), LOSS_BASE)


# --------------------------------------------------------------------------- clhip_loss_segments, C > 64
def _segments_restatement(z, y, tg, segs, T, dtype):
    """The restatement of test_gpu_icarl.py (_loss_restatement), in a chosen precision."""
    z = z.clone().to(dtype).requires_grad_(True)
    total = torch.zeros((), dtype=dtype)
    for r0, r1, o, nc, sc, kind in segs:
        zs = z[r0:r1, o:o + nc]
        if kind == 0:
            v = torch.nn.functional.cross_entropy(zs, y[r0:r1])
        else:
            v = torch.nn.KLDivLoss(reduction="batchmean")(torch.log_softmax(zs / T, 1), torch.softmax(tg[r0:r1, o:o + nc].to(dtype) / T, 1)) * T ** 2
            if float(v) < 0:
                v = v * 0
        total = total + sc * v
    total.backward()
    return total.detach().reshape(1), z.grad


def test_loss_segments_wide_slices(request):
    """A cross-entropy and a distillation segment of 130 columns each (the C > 64 branch of both kinds) at col_off 7 of 150."""
    from clsurvey_amd import ops
    gen = torch.Generator().manual_seed(41)
    N, ld, off, nc, T = 21, 150, 7, 130, 2.0
    z = torch.full((N, ld), OUTSIDE)
    tg = torch.full((N, ld), OUTSIDE)
    z[:, off:off + nc] = torch.randn((N, nc), generator=gen) * 2
    tg[:, off:off + nc] = torch.randn((N, nc), generator=gen) * 2
    y = torch.randint(0, nc, (N,), generator=gen)
    segs = [(0, 12, off, nc, 1.0, 0), (12, 21, off, nc, 2.75, 1)]
    d = dev()
    stats = torch.zeros(2, dtype=torch.float64, device=d)
    dz = torch.full((N, ld), float("nan"), device=d)
    loss, dz = ops.loss_segments(z.to(d), y.to(d), tg.to(d), ops.loss_segment_table(segs, d), len(segs), T, stats, dlogits=dz)
    torch.cuda.synchronize()
    loss, dz = loss.cpu(), dz.cpu()
    l32, g32 = _segments_restatement(z, y, tg, segs, T, torch.float32)
    l64, g64 = _segments_restatement(z, y, tg, segs, T, torch.float64)
    fp32_chain_check(request.node.name, "loss", loss, l32, l64, LOSS_BASE)
    fp32_chain_check(request.node.name, "dlogits", dz, g32, g64, LOSS_BASE)
    outside = torch.ones(ld, dtype=torch.bool)
    outside[off:off + nc] = False
    assert bool((dz[:, outside] == 0).all())
    s = stats.cpu()
    assert float(s[0]) == float(loss[0]) and float(s[1]) == float(lowest_index_hits(z[:12, off:off + nc], y[:12]))
