"""Kernel-level parity of csrc/pool.hip: clhip_maxpool2_fwd / _bwd and clhip_maxpool_fwd / _bwd (the 3x3 / stride-2 LDS pair and
the general pair) against torch's CPU F.max_pool2d(..., return_indices=True) with autograd, float32.

Values, arg-max codes (mapped to ATen's flat indices) and dx are bitwise equal to torch's.  Where the windows overlap
(stride < k) dx is also held to <= 1 ulp of an fp64 scatter that visits the windows in (oh, ow) order; those cases draw dy from
a grid of 2^-12 so every partial sum of the (at most nine) windows that meet in a pixel is exact in float32 and the bound holds
whatever the order of the additions.  The two 3x3 / stride-2 backward kernels are compared with each other bitwise on generic
(normal) dy: the same windows in the same order, so the same float32 sums.

Every tensor the kernels write lives in an arena with sentinel gaps: codes at odd byte offsets; x, y, dy, dx one float past a
16-byte boundary for the general kernels; x and dx two floats past one (8-byte aligned, not 16) for maxpool2, whose float2
accesses need no more (clhip_maxpool2_* return CLHIP_EINVAL below that, see test_pool_bn_packnet_args_cpu.py).

Sizes are the smallest that reach each branch: OH * OW = 1024 (last LDS case) and 1056 (general gather) around POOL_LDS_MAX,
OW > 32 with H < 8, one window; (k, s) with stride > k, k = 15 (the largest code), trailing rows / columns under no window;
totals past 2048 x 256 threads so the capped grids wrap.

Measured on one MI355X (every case prints `MEASURED|<test id>|<what>|<device>|<bound>` before it asserts, run with -s):
  every case: y, codes, dx differing from torch                                   0 / 0
  every overlapping case: worst dx ulp from the fp64 scatter                      0 / 1
  maxpool3s2_lds_and_general_backward_agree: dx ulp between the two kernels       0 / 0
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_parity import Arena, ByteArena, bitwise_equal, ulp_distance

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc00000
GRID_WRAP = 2048 * 256


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from clsurvey_amd import _lib
    return _lib, _lib.lib()


def out_size(n, k, s):
    return (n - k) // s + 1


def run_pool(x, dy, k, s, two=False, float_off=1):
    """x: (NC, H, W) float32, dy: (NC, OH, OW) or None (forward only).  two: the clhip_maxpool2_* entry points.
    Returns y, codes, dx (or None) as host tensors."""
    _lib, L = _L()
    NC, H, W = x.shape
    OH, OW = out_size(H, k, s), out_size(W, k, s)
    fa, ba = Arena(), ByteArena()
    kx = fa.add(x, float_off)
    ky = fa.add(NC * OH * OW, 0 if two else float_off, fill=NAN_BITS)
    kdy = fa.add(dy, 0 if two else float_off) if dy is not None else None
    kdx = fa.add(NC * H * W, float_off, fill=NAN_BITS) if dy is not None else None
    ki = ba.add(NC * OH * OW, fill=0xEE)
    fa.upload(dev())
    ba.upload(dev())
    assert fa.ptr(kx) % 16 == 4 * float_off and ba.ptr(ki) % 2 == 1
    if two:
        assert (k, s) == (2, 2) and fa.ptr(kx) % 8 == 0
        _lib.check(L.clhip_maxpool2_fwd(fa.ptr(kx), fa.ptr(ky), ba.ptr(ki), NC, H, W, _stream()), "clhip_maxpool2_fwd")
        if dy is not None:
            _lib.check(L.clhip_maxpool2_bwd(fa.ptr(kdy), ba.ptr(ki), fa.ptr(kdx), NC, H, W, _stream()), "clhip_maxpool2_bwd")
    else:
        _lib.check(L.clhip_maxpool_fwd(fa.ptr(kx), fa.ptr(ky), ba.ptr(ki), NC, H, W, k, s, _stream()), "clhip_maxpool_fwd")
        if dy is not None:
            _lib.check(L.clhip_maxpool_bwd(fa.ptr(kdy), ba.ptr(ki), fa.ptr(kdx), NC, H, W, k, s, _stream()), "clhip_maxpool_bwd")
    torch.cuda.synchronize()
    fa.download()
    ba.download()
    assert fa.gaps_untouched() and ba.gaps_untouched(), "a pool kernel wrote outside its tensors"
    assert bitwise_equal(fa.get(kx), x.reshape(-1)), "x was modified"
    if dy is not None:
        assert bitwise_equal(fa.get(kdy), dy.reshape(-1)), "dy was modified"
    return (fa.get(ky).clone().view(NC, OH, OW), ba.get(ki).clone().view(NC, OH, OW),
            fa.get(kdx).clone().view(NC, H, W) if dy is not None else None)


def aten_flat(codes, k, s, W):
    """The device's window positions r * k + c as ATen's indices into the H x W plane (as in test_maxpool_general)."""
    NC, OH, OW = codes.shape
    c = codes.long()
    oh = torch.arange(OH).view(1, OH, 1) * s
    ow = torch.arange(OW).view(1, 1, OW) * s
    return (oh + c // k) * W + ow + c % k


def reference(x, dy, k, s):
    """torch CPU float32: y, flat indices, dx by autograd; and dx by an fp64 scatter in (nc, oh, ow) order."""
    NC, H, W = x.shape
    xr = x.clone().view(1, NC, H, W).requires_grad_(dy is not None)
    y, idx = F.max_pool2d(xr, k, s, return_indices=True)
    if dy is None:
        return y.detach()[0], idx[0], None, None
    y.backward(dy.view(1, *dy.shape))
    plane = (torch.arange(NC).view(NC, 1, 1) * (H * W) + idx[0]).reshape(-1)
    dx64 = torch.zeros(NC * H * W, dtype=torch.float64).index_add_(0, plane, dy.double().reshape(-1))
    return y.detach()[0], idx[0], xr.grad[0], dx64.view(NC, H, W)


def make_inputs(seed, NC, H, W, k, s, generic_dy=False):
    """x with ties (a constant patch and values from a set of 16) so the first-maximum rule decides many windows; dy on a
    2^-12 grid where windows overlap (exact partial sums), normal otherwise."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((NC, H, W), generator=gen)
    coarse = torch.randint(-8, 8, (NC, H, W), generator=gen).float() * 0.25
    x = torch.where(torch.rand((NC, H, W), generator=gen) < 0.5, coarse, x)
    x[0, :min(H, 4), :min(W, 4)] = 0.5
    OH, OW = out_size(H, k, s), out_size(W, k, s)
    if s < k and not generic_dy:
        dy = torch.randint(-32768, 32768, (NC, OH, OW), generator=gen).float() / 4096.0
    else:
        dy = torch.randn((NC, OH, OW), generator=gen)
    return x, dy


def check_case(case, x, dy, k, s, two=False, float_off=1):
    NC, H, W = x.shape
    y, codes, dx = run_pool(x, dy, k, s, two, float_off)
    y_ref, i_ref, dx_ref, dx64 = reference(x, dy, k, s)
    assert int(codes.max()) < k * k
    flat = aten_flat(codes, k, s, W)
    bad = (int((y.view(torch.int32) != y_ref.view(torch.int32)).sum()), int((flat != i_ref).sum()),
           int((dx.view(torch.int32) != dx_ref.view(torch.int32)).sum()))
    print("MEASURED|%s|y, codes, dx differing from torch|%d %d %d|0" % ((case,) + bad))
    assert bad[0] == 0, "%d pooled values differ from ATen's" % bad[0]
    assert bad[1] == 0, "%d arg-max positions differ from ATen's" % bad[1]
    assert bad[2] == 0, "%d dx entries differ from torch's autograd" % bad[2]
    if s < k:
        ulps = ulp_distance(dx, dx64.float())
        print("MEASURED|%s|dx ulp from the fp64 scatter|%d|1" % (case, ulps))
        assert ulps <= 1, "dx is %d ulp from the fp64 scatter" % ulps
    if s > k or (H - k) % s or (W - k) % s:              # pixels under no window get exactly +0.0
        covered = torch.zeros(H, W, dtype=torch.bool)
        for r in range(k):
            for c in range(k):
                covered[r:r + (out_size(H, k, s) - 1) * s + 1:s, c:c + (out_size(W, k, s) - 1) * s + 1:s] = True
        assert not bool(covered.all())
        assert bool((dx[:, ~covered].view(torch.int32) == 0).all()), "a pixel under no window has a gradient"
    return y, codes, dx


# --------------------------------------------------------------------------- 3x3 / stride 2 around POOL_LDS_MAX
@pytest.mark.parametrize("NC", [3, 5])
@pytest.mark.parametrize("H,W", [(65, 65), (67, 65), (7, 300), (3, 3)])
def test_maxpool3s2_lds_limit(request, NC, H, W):
    """65x65: OH * OW = 1024, the last plane the LDS backward takes; 67x65: 33 x 32 = 1056, the general gather at k = 3, s = 2;
    7x300: OW = 149 > 32 (the column loop of both plane kernels runs), H < 8 (rows of threads idle); 3x3: one window."""
    OH, OW = out_size(H, 3, 2), out_size(W, 3, 2)
    assert {(65, 65): 1024, (67, 65): 1056, (7, 300): 3 * 149, (3, 3): 1}[(H, W)] == OH * OW
    x, dy = make_inputs(100 + H + W + NC, NC, H, W, 3, 2)
    check_case(request.node.name, x, dy, 3, 2)


def test_maxpool3s2_lds_and_general_backward_agree(request):
    """The same 65x65 planes through both backward kernels: once as they are (OH * OW = 1024, LDS kernel), once as the top of
    67x65 planes (1056, general gather) whose extra window row gets dy = +0.0.  Rows 0..64 of dx must agree bitwise on generic
    dy: both kernels add the windows of a pixel in (oh, ow) order, and adding +0.0 to a sum that started at +0.0 changes nothing."""
    NC = 3
    x65, dy65 = make_inputs(7, NC, 65, 65, 3, 2, generic_dy=True)
    x67 = torch.cat([x65, torch.randn((NC, 2, 65), generator=torch.Generator().manual_seed(8))], 1)
    dy67 = torch.cat([dy65, torch.zeros(NC, 1, 32)], 1)
    y65, c65, dx65 = run_pool(x65, dy65, 3, 2)
    y67, c67, dx67 = run_pool(x67, dy67, 3, 2)
    assert bitwise_equal(y65, y67[:, :32]) and torch.equal(c65, c67[:, :32])
    ulps = ulp_distance(dx65, dx67[:, :65])
    print("MEASURED|%s|dx ulp between the LDS and the general backward kernel|%d|0" % (request.node.name, ulps))
    assert bitwise_equal(dx65, dx67[:, :65].contiguous()), "the two backward kernels differ by %d ulp" % ulps
    assert bool((dx67[:, 65:].view(torch.int32) == 0).all())
    _, _, dx_ref, _ = reference(x65, dy65, 3, 2)
    assert bitwise_equal(dx65, dx_ref), "generic dy: dx differs from torch's autograd"


# --------------------------------------------------------------------------- general kernels
GENERAL = [  # k, s, H, W: trailing rows and columns under no window wherever the geometry allows one
    (2, 3, 12, 13), (1, 1, 5, 7), (5, 3, 18, 21), (3, 1, 9, 11), (4, 4, 14, 19), (15, 7, 40, 33)]


@pytest.mark.parametrize("k,s,H,W", GENERAL)
def test_maxpool_general_kernels(request, k, s, H, W):
    x, dy = make_inputs(200 + 16 * k + s, 3, H, W, k, s)
    if k == 15:
        x[1, 14:29, 7:22] = -3.0                           # the last position of a 15 x 15 window wins: code 224
        x[1, 28, 21] = 9.0
    y, codes, dx = check_case(request.node.name, x, dy, k, s)
    if k == 15:
        assert int(codes[1, 2, 1]) == 224


def test_maxpool_general_grid_wraps(request):
    """NC = 9, 2x2 / 1 on 250x250: 9 * 249 * 249 outputs and 9 * 250 * 250 inputs, both past 2048 x 256 threads."""
    NC, H, W, k, s = 9, 250, 250, 2, 1
    assert NC * out_size(H, k, s) * out_size(W, k, s) > GRID_WRAP and NC * H * W > GRID_WRAP
    x, dy = make_inputs(31, NC, H, W, k, s)
    check_case(request.node.name, x, dy, k, s)


def test_maxpool2_grid_wraps(request):
    """NC = 9 on 500x500: 9 * 250 * 250 windows past 2048 x 256 threads; x and dx 8-byte aligned only."""
    NC, H, W = 9, 500, 500
    assert NC * (H // 2) * (W // 2) > GRID_WRAP
    x, dy = make_inputs(32, NC, H, W, 2, 2)
    check_case(request.node.name, x, dy, 2, 2, two=True, float_off=2)


@pytest.mark.parametrize("NC,H,W", [(1, 2, 2), (3, 6, 10), (5, 34, 18)])
@pytest.mark.parametrize("float_off", [0, 2])
def test_maxpool2_small(request, NC, H, W, float_off):
    x, dy = make_inputs(300 + H + W, NC, H, W, 2, 2)
    y, codes, dx = check_case(request.node.name, x, dy, 2, 2, two=True, float_off=float_off)
    y1, codes1, dx1 = run_pool(x, dy, 2, 2)                # the general kernels at k = 2, s = 2: the same operator
    assert bitwise_equal(y, y1) and torch.equal(codes, codes1) and bitwise_equal(dx, dx1)


# --------------------------------------------------------------------------- scan-order edges
def _f(bits):
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32)[0].item()


NAN, INF = float("nan"), float("inf")
DEN = _f(0x00000001)            # the smallest positive denormal
DEN_BIG = _f(0x007fffff)        # the largest
LOW = -5.0                      # below every finite value of the patterns


def edge_patterns(L):
    """(name, the window's first values in scan order (the rest is LOW, or the pattern's own filler), expected code).  L: the
    window's size (4 or 9)."""
    def pad(v, fill=LOW):
        return list(v) + [fill] * (L - len(v))
    return [
        ("all equal", pad([1.0] * L), 0),
        ("-0.0 before +0.0", pad([-0.0, 0.0]), 0),
        ("+0.0 before -0.0", pad([0.0, -0.0]), 0),
        ("-0.0 after a lower value, then +0.0", pad([LOW, -0.0, 0.0]), 1),
        ("NaN first", pad([NAN, 1.0, 2.0]), 0),
        ("NaN last", pad([2.0, 1.0])[:L - 1] + [NAN], L - 1),
        ("two NaNs", pad([NAN, 1.0, NAN]), 2),
        ("all -inf", [-INF] * L, 0),
        ("-inf, then a finite value", pad([-INF, -INF, LOW], -INF), 2),
        ("+inf before NaN", pad([INF, NAN]), 1),
        ("NaN before +inf", pad([NAN, INF]), 0),
        ("+inf twice", pad([1.0, INF, INF]), 1),
        ("denormals of both signs", pad([-DEN, DEN, 0.0, -0.0][:min(L, 4)]), 1),
        ("negative denormals", pad([-DEN_BIG, -DEN, -DEN]), 1),
        ("positive denormals", pad([DEN, DEN_BIG, DEN_BIG]), 1),
        ("denormal against zero", pad([0.0, DEN, -DEN]), 1),
    ]


@functools.lru_cache(maxsize=None)
def edge_plane(k, pitch):
    """One k x k tile per pattern at `pitch`, rows of 4 tiles; the rest of the plane is LOW."""
    pats = edge_patterns(k * k)
    rows = (len(pats) + 3) // 4
    H, W = (rows - 1) * pitch + k, 3 * pitch + k
    if k == 2:
        H, W = H + H % 2, W + W % 2
    x = torch.full((1, H, W), LOW)
    where = []
    for i, (_, vals, _) in enumerate(pats):
        r0, c0 = (i // 4) * pitch, (i % 4) * pitch
        x[0, r0:r0 + k, c0:c0 + k] = torch.tensor(vals, dtype=torch.float32).view(k, k)
        where.append((r0, c0))
    return x, where


@pytest.mark.parametrize("kernel", ["maxpool2", "general-2x2", "plane-3x3s2", "general-3x3s4"])
def test_scan_order_edges(request, kernel):
    """Hand-placed windows through the three forward kernels (the general one at both window sizes): the code is the one the
    scan rule `v > m || v != v` gives by hand, and values and codes are ATen's for every window of the plane."""
    k, s, pitch, two = {"maxpool2": (2, 2, 2, True), "general-2x2": (2, 2, 2, False), "plane-3x3s2": (3, 2, 4, False),
                        "general-3x3s4": (3, 4, 4, False)}[kernel]
    x, where = edge_plane(k, pitch)
    x = x.repeat(2, 1, 1)
    NC, H, W = x.shape
    y, codes, _ = run_pool(x, None, k, s, two, 2 if two else 1)
    y_ref, i_ref, _, _ = reference(x, None, k, s)
    wrong = []
    for (name, vals, want), (r0, c0) in zip(edge_patterns(k * k), where):
        for nc in range(NC):
            got = int(codes[nc, r0 // s, c0 // s])
            v = y[nc, r0 // s, c0 // s].view(1)
            if got != want or not bitwise_equal(v, torch.tensor([vals[want]], dtype=torch.float32)):
                wrong.append("%s: code %d value %r, by hand code %d value %r" % (name, got, float(v), want, vals[want]))
    print("MEASURED|%s|hand-placed windows with another code or value|%d|0" % (request.node.name, len(wrong)))
    assert not wrong, "\n".join(wrong)
    assert bitwise_equal(y, y_ref), "values differ from ATen's"
    assert torch.equal(aten_flat(codes, k, s, W), i_ref), "arg-max positions differ from ATen's"
