"""LwF / EBLL on heads of any size, without a GPU: the entry points of csrc/lwf_wide.hip (exported, declared, bound; the
workspace size; every refusal, reached with dummy pointers that are never dereferenced because nothing is launched), the
packed runs of ParamArena on the CPU, and the plan lwf_plan returns for a CPU wrapper."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

EINVAL, ENOSPC = -1, -2
WIDE_MAX = 64                # CLHIP_LWF_MAX_HEADS_WIDE
HERE = os.path.dirname(os.path.abspath(__file__))


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    return _lib, L, C.addressof(buf), buf


def _pad4(n):
    return (n + 3) // 4 * 4


def test_wide_entries_are_exported_declared_and_bound():
    _lib, L, p, _keep = _setup()
    with open(os.path.join(HERE, "..", "include", "clhip.h")) as f:
        header = f.read()
    for name in ("clhip_lwf_loss_wide_ws", "clhip_lwf_loss_wide"):
        assert getattr(L, name) is not None                                          # exported
        assert re.search(r"\b%s\(" % name, header), name                            # declared
        assert name in _lib.SIGNATURES                                               # bound
    assert re.search(r"#define\s+CLHIP_LWF_MAX_HEADS_WIDE\s+64\b", header)
    assert _lib.SIGNATURES["clhip_lwf_loss_wide_ws"] == (C.c_size_t, [C.c_int, C.c_int])
    assert len(_lib.SIGNATURES["clhip_lwf_loss_wide"][1]) == 17
    from clsurvey_amd import build
    assert "lwf_wide.hip" in build.SOURCES


def test_wide_ws_size():
    _lib, L, p, _keep = _setup()
    for n_heads in (0, 65, -1):
        assert L.clhip_lwf_loss_wide_ws(n_heads, 8) == 0, n_heads
    for N in (0, 1025, -1):
        assert L.clhip_lwf_loss_wide_ws(3, N) == 0, N
    for n_heads in (1, 2, 33, 64):
        for N in (1, 2, 3, 4, 5, 37, 200, 1023, 1024):
            need = L.clhip_lwf_loss_wide_ws(n_heads, N)
            assert need > 0 and need % 16 == 0, (n_heads, N, need)
            assert need >= 3 * 4 * N, (n_heads, N, need)                             # (task, distillation, hit) per row


def _caller(L, p):
    def call(sizes, N=4, ld=None, ld_t=None, T=2.0, distill=1, teacher=p, n_heads=None, ws=p, ws_bytes=None, null=None):
        hs = (C.c_int * max(len(sizes), 1))(*sizes)
        n = len(sizes) if n_heads is None else n_heads
        ld = sum(sizes) if ld is None else ld
        ld_t = sum(sizes[:-1]) if ld_t is None else ld_t
        if ws_bytes is None:
            ws_bytes = 1 << 20
        # (logits, labels, teacher, head_sizes, n_heads, N, ld, ld_t, T, lambda, distill, dlogits, loss2, stats, ws, ws_bytes, stream)
        a = [p, p, teacher, hs, n, N, ld, ld_t, T, 1.0, distill, p, p, None, ws, ws_bytes, None]
        if null is not None:
            a[null] = None
        return L.clhip_lwf_loss_wide(*a)
    return call


def test_wide_refusals():
    _lib, L, p, _keep = _setup()
    call = _caller(L, p)
    for null in (0, 1, 3, 11, 12, 14):                                               # logits, labels, head_sizes, dlogits, loss2, ws
        assert call([4, 4], null=null) == EINVAL, null
    assert call([], n_heads=0) == EINVAL
    assert call([1] * 65) == EINVAL
    assert call([1] * 64, n_heads=-1) == EINVAL
    assert call([4, 0, 4]) == EINVAL                                                 # an empty head
    assert call([4, -3, 4], ld=64) == EINVAL
    assert call([8, 9], ld=16) == EINVAL                                             # heads wider than ld
    assert call([8, 4], ld=16, ld_t=7) == EINVAL                                     # old heads wider than ld_teacher
    assert call([4, 4], N=0) == EINVAL
    assert call([4, 4], N=1025) == EINVAL
    assert call([4, 4], T=0.0) == EINVAL
    assert call([4, 4], T=-1.0) == EINVAL
    assert call([4, 4], teacher=None) == EINVAL                                      # two heads distilled from no teacher
    need = L.clhip_lwf_loss_wide_ws(2, 4)
    assert call([4, 4], ws_bytes=need - 1) == ENOSPC
    assert call([4, 4], ws_bytes=0) == ENOSPC


def test_wide_refusals_come_in_the_documented_order():
    """The header lists the argument checks before the workspace check: every bad argument is CLHIP_EINVAL even when the
    workspace is too small as well, and the workspace is only measured (N and n_heads are known to be in range by then)
    once everything else holds.  Among the CLHIP_EINVAL checks the order shows where a later check would read what an
    earlier one guards: the sizes are summed only for n_heads in range (65 sizes do not fit the kernel's table)."""
    _lib, L, p, _keep = _setup()
    call = _caller(L, p)
    short = dict(ws_bytes=0)
    assert call([4, 4], null=0, **short) == EINVAL
    assert call([1] * 65, **short) == EINVAL
    assert call([4, 0, 4], **short) == EINVAL
    assert call([8, 9], ld=16, **short) == EINVAL
    assert call([8, 4], ld=16, ld_t=7, **short) == EINVAL
    assert call([4, 4], N=1025, **short) == EINVAL
    assert call([4, 4], T=0.0, **short) == EINVAL
    assert call([4, 4], teacher=None, **short) == EINVAL
    assert call([4, 4], **short) == ENOSPC
    # n_heads far out of range with a size table of one entry: refused before any size is read
    assert call([4], n_heads=1 << 20) == EINVAL
    # distill = 0 (validation) and a single head need neither a teacher nor its row stride
    assert call([4, 4], distill=0, teacher=None, ld_t=0, null=0) == EINVAL           # still refused, for the NULL logits alone
    assert call([4], teacher=None, ld_t=0, ws_bytes=0) == ENOSPC                     # one head: every argument check passes


def test_wide_workspace_checks_at_64_heads():
    _lib, L, p, _keep = _setup()
    call = _caller(L, p)
    sizes = [(5 * i) % 9 + 1 for i in range(WIDE_MAX)]
    for N in (1, 37, 1024):
        need = L.clhip_lwf_loss_wide_ws(WIDE_MAX, N)
        assert need > 0
        assert call(sizes, N=N, ws=None, ws_bytes=need) == EINVAL                    # a sufficient size, no workspace
        assert call(sizes, N=N, ws_bytes=need - 1) == ENOSPC                         # one byte short


# --------------------------------------------------------------------------------------------- ParamArena on the CPU
def _params(shapes, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]


def test_param_arena_without_runs_is_the_pad_to_4_layout():
    from clsurvey_amd.net import ParamArena
    shapes = [(3, 3, 3, 3), (3,), (5, 7), (5,), (6, 5), (6,), (1,), (2, 2)]
    ps = _params(shapes)
    values = [p.detach().clone() for p in ps]
    a = ParamArena(ps, device="cpu")
    off, want = 0, []
    for p in ps:
        want.append(off)
        off += _pad4(p.numel())
    assert a.offsets == want and a.numel == off and a.runs is None
    b = ParamArena(_params(shapes), device="cpu", runs=None)
    assert b.offsets == want and b.numel == off
    for p, v in zip(ps, values):
        assert torch.equal(p.data, v)


def test_param_arena_packed_runs():
    from clsurvey_amd.net import ParamArena
    feat = 7
    shapes = [(3, 2), (3,), (5, feat), (3, feat), (6, feat), (5,), (3,), (6,), (9,), (2,)]
    ps = _params(shapes, seed=1)
    values = [p.detach().clone() for p in ps]
    a = ParamArena(ps, device="cpu", runs=[(2, 3), (5, 3)])
    assert a.offsets[0] == 0 and a.offsets[1] == 8                                   # in front of the runs: pad to 4
    w = a.offsets[2]
    assert w == 12 and w % 4 == 0
    assert a.offsets[2:5] == [w, w + 5 * feat, w + 8 * feat]                         # head weights back to back
    o = a.offsets[5]
    assert o == _pad4(w + 14 * feat) and o % 4 == 0
    assert a.offsets[5:8] == [o, o + 5, o + 8]                                       # head biases back to back
    assert a.offsets[8] == o + 16                                                    # 14 floats, padded to 4: the next slot
    assert a.offsets[9] == o + 16 + 12 and a.numel == o + 16 + 12 + 4
    for p, v, off in zip(ps, values, a.offsets):
        assert torch.equal(p.data, v)
        assert p.data.data_ptr() == a.theta.data_ptr() + 4 * off
        assert p.grad.data_ptr() == a.grad.data_ptr() + 4 * off and p.grad.shape == p.shape
        assert a.slot(p) == (off, p.numel())
    # the run read as one tensor is the concatenation of its parameters
    assert torch.equal(a.theta[o:o + 14], torch.cat([v.reshape(-1) for v in values[5:8]]))
    assert torch.equal(a.theta[w:w + 14 * feat].view(14, feat), torch.cat(values[2:5], 0))
    ps[6].grad.fill_(2.5)                                                            # p.grad aliases the grad arena
    assert torch.equal(a.grad[o + 5:o + 8], torch.full((3,), 2.5)) and float(a.grad.sum()) == 7.5
    a.zero_grad()
    assert float(ps[6].grad.abs().sum()) == 0.0
    a.load("omega", {ps[6]: torch.full((3,), 4.0)})
    assert torch.equal(a.view("omega", ps[6]), torch.full((3,), 4.0)) and float(a.aux["omega"].sum()) == 12.0
    assert float(a.aux["omega"][o + 5]) == 4.0 and float(a.aux["omega"][o + 4]) == 0.0
    with pytest.raises(ValueError):
        ParamArena(_params(shapes), device="cpu", runs=[(2, 3), (4, 3)])             # overlapping
    with pytest.raises(ValueError):
        ParamArena(_params(shapes), device="cpu", runs=[(8, 3)])                     # past the end


# --------------------------------------------------------------------------------------------- lwf_plan on a CPU wrapper
def _wrapper(sizes):
    from clsurvey_amd import models
    from clsurvey_amd.methods import lwf as LF
    tiny = [16, "M", 16, "M", 32, 32, "M", 32, 32, "M"]
    m = models.VGGSlim(cfg=tiny, num_classes=sizes[0], classifier_inputdim=32 * 2 * 2, classifier_dim1=24, classifier_dim2=24)
    w = LF.AlexNet_LwF(m, last_layer_name=4)
    for i, nc in enumerate(sizes[1:]):
        w.model.classifier.add_module(str(5 + i), nn.Linear(24, nc))
    return w


def test_lwf_plan_any_head_size():
    from clsurvey_amd.methods import lwf as LF
    layers, params, sizes, drops, runs = LF.lwf_plan(_wrapper([5, 3, 6]))            # raised NotImplementedError before
    assert sizes == [5, 3, 6]
    n = len(params)
    assert runs == [(n - 6, 3), (n - 3, 3)]
    assert [tuple(p.shape) for p in params[n - 6:]] == [(5, 24), (3, 24), (6, 24), (5,), (3,), (6,)]
    assert layers[-1][0] == "fc" and layers[-1][3:5] == (24, 14)
    assert layers[-1][1] is params[n - 6] and layers[-1][2] is params[n - 3]          # the plan uses the first of each run


def test_lwf_plan_keeps_the_accepted_plans_unpacked():
    from clsurvey_amd.methods import lwf as LF
    layers, params, sizes, drops, runs = LF.lwf_plan(_wrapper([8, 4, 4]))
    assert sizes == [8, 4, 4] and runs is None
    assert LF.lwf_plan(_wrapper([4] * 32))[4] is None                                # 32 heads: clhip_lwf_loss still takes them
    assert LF.lwf_plan(_wrapper([4] * 33))[4] is not None                            # 33: packed or not, the wide kernel's


def test_lwf_plan_refuses_65_heads_naming_the_limit():
    from clsurvey_amd.methods import lwf as LF
    assert len(LF.lwf_plan(_wrapper([2] * 64))[2]) == 64
    with pytest.raises(NotImplementedError, match="CLHIP_LWF_MAX_HEADS_WIDE"):
        LF.lwf_plan(_wrapper([2] * 65))
