"""Kernel-level parity of csrc/lwf_wide.hip: clhip_lwf_loss_wide against oracle.lwf_ref.lwf_objective evaluated in fp64 and in
float32 on the CPU from the same float32 inputs (kernel_parity.fp32_chain_check with LOSS_BASE, the rule and the bound of
test_lwf_loss_against_fp64 for clhip_lwf_loss: the formulas are the same, only the order of the row sums differs).

Layouts (the lanes of a wave run across the columns of a head, 64 at a time; one wave per row, 4 rows per block):
  one      [5]                                          no old head, no teacher
  two      [3, 4]
  lanes    [1, 63, 64, 65, 129, 2]                      the lane boundaries: 64 is the last single-pass head, 129 takes three
  recogseq [102, 67, 200, 196, 100, 11, 52, 11]         the reference's RecogSeq sequence (739 columns)
  forty    [5] * 40                                     the long Tiny-ImageNet sequence
  max      [(5 i) % 9 + 1 for i < 64]                   CLHIP_LWF_MAX_HEADS_WIDE heads
  past32   33 heads of 1..3 classes, the last of 2      first length past clhip_lwf_loss
N = 1 leaves three waves of the only block without a row, 37 is no multiple of 4, 1024 is the limit.  Odd ld / ld_teacher
(logit padding 3, teacher padding 5) leave every row after the first unaligned.  Counts, zeros and the statistics'
accumulation are exact; two calls agree bitwise (no atomics, one summation order).
"""
import ctypes as C

import pytest
import torch

from kernel_parity import LOSS_BASE, bitwise_equal, fp32_chain_check, ulp_distance
from oracle import lwf_ref

pytestmark = pytest.mark.gpu

OUTSIDE = 1.0e4          # logits / teacher columns past the heads: larger than anything inside, so a leak shows at once
EINVAL, ENOSPC = -1, -2

HEADS = {
    "one": [5],
    "two": [3, 4],
    "lanes": [1, 63, 64, 65, 129, 2],
    "recogseq": [102, 67, 200, 196, 100, 11, 52, 11],
    "forty": [5] * 40,
    "max": [(5 * i) % 9 + 1 for i in range(64)],
    "past32": [i % 3 + 1 for i in range(32)] + [2],
    "many32": [(5 * i) % 9 + 1 for i in range(32)],          # both kernels take it
}
CASES = [
    # N, layout, T, lam, distill, teacher columns past the old heads, logit columns past the heads
    (1, "one", 1.0, 0.5, 1, 0, 0), (37, "one", 2.0, 10.0, 0, 0, 3), (1024, "one", 4.0, 0.5, 1, 0, 3),
    (1, "two", 2.0, 10.0, 1, 0, 3), (37, "two", 1.0, 0.5, 1, 5, 0), (1024, "two", 4.0, 10.0, 0, 0, 3),
    (1, "lanes", 4.0, 0.5, 1, 5, 3), (37, "lanes", 2.0, 10.0, 1, 0, 3), (1024, "lanes", 1.0, 0.5, 1, 5, 0),
    (1, "recogseq", 1.0, 10.0, 1, 0, 0), (37, "recogseq", 4.0, 0.5, 1, 5, 3), (1024, "recogseq", 2.0, 10.0, 1, 0, 3),
    (37, "recogseq", 2.0, 10.0, 0, 5, 3),
    (1, "forty", 2.0, 0.5, 1, 5, 3), (37, "forty", 1.0, 10.0, 1, 0, 3), (1024, "forty", 4.0, 0.5, 1, 5, 0),
    (1, "max", 4.0, 10.0, 1, 0, 0), (37, "max", 2.0, 0.5, 1, 5, 3), (1024, "max", 1.0, 10.0, 1, 0, 3),
    (37, "max", 2.0, 10.0, 0, 5, 3),
    (1, "past32", 1.0, 0.5, 1, 5, 3), (37, "past32", 4.0, 10.0, 1, 0, 3), (1024, "past32", 2.0, 0.5, 1, 5, 0),
]


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def lowest_index_hits(zs, y):
    """#rows whose label is the FIRST column attaining the row maximum (torch.max's rule), spelled out without an arg-max."""
    m = zs.max(1, keepdim=True).values
    idx = torch.arange(zs.shape[1]).expand_as(zs)
    first = torch.where(zs == m, idx, torch.full_like(idx, zs.shape[1])).min(1).values
    return int((first == y).sum())


def problem(sizes, N, t_pad, z_pad, seed=21):
    width, old = sum(sizes), sum(sizes[:-1])
    ld, ld_t = width + z_pad, old + t_pad
    gen = torch.Generator().manual_seed(seed)
    z = torch.full((N, ld), OUTSIDE)
    z[:, :width] = torch.randn((N, width), generator=gen) * 3
    y = torch.randint(0, sizes[-1], (N,), generator=gen)
    teacher = None
    if len(sizes) > 1:                                # a single head has nothing to distil: teacher stays NULL
        teacher = torch.full((N, ld_t), OUTSIDE)
        teacher[:, :old] = torch.randn((N, old), generator=gen) * 3
    return z, y, teacher


def reference(z, y, teacher, sizes, T, lam, distill, dtype):
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


_REFS = {}


def references(key, z, y, teacher, sizes, T, lam, distill):
    """(float32, fp64) references of one problem, computed once and shared by the tests that use the same problem."""
    if key not in _REFS:
        _REFS[key] = (reference(z, y, teacher, sizes, T, lam, distill, torch.float32),
                      reference(z, y, teacher, sizes, T, lam, distill, torch.float64))
    return _REFS[key]


SEED_STATS = [1.5, 3.0]


def run(entry, z, y, teacher, sizes, T, lam, distill, calls=1):
    """One (or `calls` consecutive) launches of `entry` ('wide' | 'narrow') on NaN-poisoned outputs and seeded statistics."""
    from clsurvey_amd import _lib
    L = _lib.lib()
    N, ld = z.shape
    ld_t = teacher.shape[1] if teacher is not None else 0
    d = dev()
    zd, yd = z.to(d), y.to(d)
    td = teacher.to(d) if teacher is not None else None
    hs = (C.c_int * len(sizes))(*sizes)
    out = []
    for _ in range(calls):
        dz = torch.full((N, ld), float("nan"), device=d)
        loss2 = torch.full((2,), float("nan"), device=d)
        stats = torch.tensor(SEED_STATS, dtype=torch.float64, device=d)
        args = (zd.data_ptr(), yd.data_ptr(), td.data_ptr() if td is not None else None, hs, len(sizes), N, ld, ld_t, T, lam, distill,
                dz.data_ptr(), loss2.data_ptr(), stats.data_ptr())
        stream = torch.cuda.current_stream().cuda_stream
        if entry == "wide":
            need = L.clhip_lwf_loss_wide_ws(len(sizes), N)
            assert need > 0 and need % 16 == 0
            ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=d)
            _lib.check(L.clhip_lwf_loss_wide(*args, ws.data_ptr(), need, stream), "clhip_lwf_loss_wide")
        else:
            _lib.check(L.clhip_lwf_loss(*args, stream), "clhip_lwf_loss")
        torch.cuda.synchronize()
        out.append((loss2.cpu(), dz.cpu(), stats.cpu()))
    return out[0] if calls == 1 else out


def check(case, got, refs, z, y, sizes, distill):
    loss2, dz, stats = got
    (l32, g32), (l64, g64) = refs
    width, old = sum(sizes), sum(sizes[:-1])
    fp32_chain_check(case, "task loss", loss2[0:1], l32[0:1], l64[0:1], LOSS_BASE)
    if distill and len(sizes) > 1:
        fp32_chain_check(case, "lambda * distillation", loss2[1:2], l32[1:2], l64[1:2], LOSS_BASE)
    else:
        assert float(loss2[1]) == 0.0
    fp32_chain_check(case, "dlogits", dz, g32, g64, LOSS_BASE)
    assert bool((dz[:, width:] == 0).all()), "dlogits past the last head must be exactly 0"
    if not distill:
        assert bool((dz[:, :old] == 0).all()), "distill = 0: no gradient on the old heads"
    assert float(stats[0]) == SEED_STATS[0] + float(loss2[0])
    assert float(stats[1]) == SEED_STATS[1] + lowest_index_hits(z[:, old:width], y)


@pytest.mark.parametrize("N,layout,T,lam,distill,t_pad,z_pad", CASES, ids=["%d-%s-T%g-lam%g-d%d-tp%d-zp%d" % c for c in CASES])
def test_lwf_loss_wide_against_fp64(request, N, layout, T, lam, distill, t_pad, z_pad):
    sizes = HEADS[layout]
    assert 1 <= len(sizes) <= 64 and min(sizes) >= 1
    z, y, teacher = problem(sizes, N, t_pad, z_pad)
    a, b = run("wide", z, y, teacher, sizes, T, lam, distill, calls=2)
    refs = references((N, layout, T, lam, distill, t_pad, z_pad), z, y, teacher, sizes, T, lam, distill)
    check(request.node.name, a, refs, z, y, sizes, distill)
    for what, u, v in zip(("loss2", "dlogits", "stats"), a, b):
        if what == "stats":
            assert torch.equal(u, v), "two calls on the same inputs: stats differ"
        else:
            assert bitwise_equal(u, v), "two calls on the same inputs: %s differs bitwise" % what


TIE_PAIRS = [(0, 1), (63, 64), (64, 128)]


@pytest.mark.parametrize("mode", ["first", "second"])
def test_lwf_loss_wide_tie_rule_lowest_index(mode):
    """A last head of 130 classes whose first rows attain their maximum at two columns with identical float32 values: two
    columns of one lane pass (0, 1), the last lane of the first pass and the first of the second (63, 64), and lane 0's
    first and third column (64, 128: the lane's own strict `>` keeps 64).  Only `label == first tied column` counts as
    correct (torch.max's lowest-index rule): with the label on the first tied column every tied row is a hit, with it on
    the second none is."""
    sizes = [3, 130]
    N, old = 37, 3
    z, y, teacher = problem(sizes, N, 5, 3, seed=23)
    rows = 4 * len(TIE_PAIRS)
    for r in range(rows):
        cols = TIE_PAIRS[r % len(TIE_PAIRS)]
        for c in cols:
            z[r, old + c] = 50.0
        y[r] = cols[0 if mode == "first" else 1]
    zs = z[:, old:old + 130]
    hits = lowest_index_hits(zs, y)
    untied = lowest_index_hits(zs[rows:], y[rows:])
    assert hits == untied + (rows if mode == "first" else 0)             # the rule, stated without any arg-max
    loss2, dz, stats = run("wide", z, y, teacher, sizes, 2.0, 1.0, 1)
    assert float(stats[1]) == SEED_STATS[1] + hits, "correct-count %r, lowest-index rule %d (%d tied rows, label on the %s tied column)" % (
        float(stats[1]) - SEED_STATS[1], hits, rows, mode)
    refs = references(("tie", mode), z, y, teacher, sizes, 2.0, 1.0, 1)
    check("tie-" + mode, (loss2, dz, stats), refs, z, y, sizes, 1)


@pytest.mark.parametrize("layout,N", [("two", 37), ("recogseq", 200), ("many32", 200)])
def test_both_kernels_on_the_layouts_both_take(layout, N):
    """clhip_lwf_loss and clhip_lwf_loss_wide pass the same check against the same references; their distance is printed, not
    asserted to be 0: the row sums run in another order (lanes + butterfly instead of one thread in column order)."""
    sizes = HEADS[layout]
    assert len(sizes) <= 32
    T, lam = 2.0, 10.0
    z, y, teacher = problem(sizes, N, 5, 3, seed=29)
    refs = references(("both", layout, N), z, y, teacher, sizes, T, lam, 1)
    narrow = run("narrow", z, y, teacher, sizes, T, lam, 1)
    wide = run("wide", z, y, teacher, sizes, T, lam, 1)
    check("both-%s-narrow" % layout, narrow, refs, z, y, sizes, 1)
    check("both-%s-wide" % layout, wide, refs, z, y, sizes, 1)
    print("MEASURED|both-%s|ulp distance wide vs narrow: dlogits %d, loss2 %d" % (
        layout, ulp_distance(wide[1], narrow[1]), ulp_distance(wide[0], narrow[0])))
    assert float(wide[2][1]) == float(narrow[2][1])                      # the hit count is exact in both


def test_refused_calls_write_nothing():
    from clsurvey_amd import _lib
    L = _lib.lib()
    sizes = [3, 4]
    N, ld, ld_t = 5, 10, 4
    d = dev()
    z = torch.randn(N, ld, device=d)
    y = torch.zeros(N, dtype=torch.int64, device=d)
    t = torch.randn(N, ld_t, device=d)
    dz = torch.full((N, ld), float("nan"), device=d)
    loss2 = torch.full((2,), float("nan"), device=d)
    stats = torch.tensor(SEED_STATS, dtype=torch.float64, device=d)
    need = L.clhip_lwf_loss_wide_ws(2, N)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=d)
    stream = torch.cuda.current_stream().cuda_stream

    def call(sizes=sizes, N=N, ld=ld, ld_t=ld_t, T=2.0, teacher=t.data_ptr(), ws_bytes=need):
        hs = (C.c_int * len(sizes))(*sizes)
        return L.clhip_lwf_loss_wide(z.data_ptr(), y.data_ptr(), teacher, hs, len(sizes), N, ld, ld_t, T, 1.0, 1, dz.data_ptr(),
                                     loss2.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    assert call(sizes=[3, 0]) == EINVAL
    assert call(sizes=[3, 8]) == EINVAL                                  # wider than ld
    assert call(ld_t=2) == EINVAL
    assert call(N=0) == EINVAL
    assert call(T=0.0) == EINVAL
    assert call(teacher=None) == EINVAL
    assert call(ws_bytes=need - 1) == ENOSPC
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz).all()) and bool(torch.isnan(loss2).all())
    assert stats.cpu().tolist() == SEED_STATS
    assert bool((ws == 0xA5).all())
    assert call() == 0                                                   # the same buffers, accepted: everything is written
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(loss2).all())
