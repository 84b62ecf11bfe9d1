"""The backward-data kernels that un-pool while they stage (arg-max codes given: dy is the gradient of the POOLED output) load each
pooled gradient and code once per window (row) and write the window's pixels from it (csrc/stage_map.hpp) where they used to load
them once per un-pooled halo pixel.  The LDS image they build must not change by a bit, so every such entry point must be BITWISE
equal to the two-step path it fuses: clhip_maxpool2_bwd of (pooled gradient, codes), then the plain backward-data entry of the same
kernel family, which stages the un-pooled gradient as it always did and runs the same matrix code on it.

Codes: uniform in 0..3, about a quarter of them then set to 4 (the fused forward's `no positive maximum`: the window passes nothing).

Shapes, (N, K = channels of dy, C = channels of dx, H, W) — the smallest that reach every branch of the new staging:
  bf16-split   32 x 32 (the 32 x 4 tile: 8 tiles per image, first / interior / last), 16 x 16 (16 x 8), 8 x 8 (two images per block;
               N = 3: the last block's second image lies past the batch), 8 x 64 (32-wide tiles on an 8-row map: the tiles' lower
               halves lie below the image), and the two-geometry launch at the smallest N that bs_launch_mixed32 takes at 32 x 32
               (tests/bs_dispatch.py: 97), through clhip_conv3x3_bs_bwd_data and clhip_conv3x3_bs_bwd_data_riders.
               K = 32 (two 16-channel chunks) is the fewest channels of dy the path takes: clhip_internal_bs_ok refuses K = 16
               (asserted below), so the one-chunk case of a 16-channel dy does not exist for this kernel.
  wino_conv16g 16 x 16 and 32 x 32 (<8, 2, 4>; N = 3) with K = 16 and 24: four and six 4-channel chunks, the fewest the Winograd path
               takes (K % 8 == 0, K >= 16, so a one-chunk or odd-chunk launch does not exist) and a count that is no multiple of four;
               8 x 8 (<4, 4, 4>, two images per block) at N = 161, C = 256: launch_wino gives 8 x 8 maps to this kernel only from 640
               units of the one-image kernel on (N = 160 at 256 channels), and the odd N leaves the last block one image past the
               batch; the merged grid clhip_conv3x3_wino_bwd at 16 x 16 (N = 3) and at 8 x 8 with N * ceil(C / 32) > 512 (N = 129,
               C = 128: below that its backward-data half is wino_conv16_body, which this change leaves alone) — dx, dw and db
               against the same grid on the un-pooled gradient: the two-step rule of this file applied to the merged entry.  (The
               merged grid against the two LAUNCHES it merges is tests/test_gpu_pair.py's subject and is not repeated here.)
  wino_conv16  the one-image 8 x 8 kernel; its un-pooling instances keep the per-element staging, the cases pass on them as they are and
               hold any later change of that staging to the same results: K = 16, KT2 = 1 at N = 3 (C = 32) and KT2 = 2 at the smallest N
               for which launch_wino picks it with 128 channels (N = 129: N * ceil(C / 32) > 512); the merged grid at 8 x 8 with N = 3,
               whose backward-data half is wino_conv16_body<1, UNPOOL, 1>.
  plain 8 x 8  forward (bias + ReLU) and backward-data (with the ReLU mask) of wino_conv16_kernel, both KT2, against SHA-256 digests of
               the outputs recorded from the parent commit's build (tests/golden/unpool_once_plain8x8.json; inputs from numpy's
               RandomState, whose stream is frozen across versions; their digests are recorded too, so that a changed input shows as such
               and not as a kernel difference; every case also with the input tensor 4 bytes off a 16-byte boundary).  No other entry computes these sums in this order, hence recorded values."""
import hashlib
import json
import os

import pytest

import bs_dispatch

pytestmark = pytest.mark.gpu


def _inputs(N, K, C, H, W, seed):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn((N, K, H // 2, W // 2), generator=g)
    idx = torch.randint(0, 4, dy.shape, generator=g)
    idx[torch.rand(dy.shape, generator=g) < 0.25] = 4
    w = torch.randn((K, C, 3, 3), generator=g) * 0.05
    src = torch.randn((N, C, H, W), generator=g)
    return dy.to(dev), idx.to(torch.uint8).to(dev), w.to(dev), src.to(dev)


def _unpooled(L, dy, idx, H, W):
    """max_pool2d backward as a launch of its own"""
    import torch
    N, K = dy.shape[:2]
    full = torch.full((N, K, H, W), 3.0, device=dy.device)
    assert L.clhip_maxpool2_bwd(dy.data_ptr(), idx.data_ptr(), full.data_ptr(), N * K, H, W, None) == 0
    return full


BS_SHAPES = [(3, 32, 64, 32, 32), (3, 32, 64, 16, 16), (3, 32, 64, 8, 8), (2, 32, 64, 8, 64)]


@pytest.mark.parametrize("shape", BS_SHAPES, ids=lambda s: "n%d_k%d_c%d_%dx%d" % s)
def test_bs_unpooling_equals_two_steps(shape):
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    N, K, C, H, W = shape
    dy, idx, w, src = _inputs(N, K, C, H, W, 40)
    ws = torch.empty(L.clhip_conv3x3_bs_ws(C, K), dtype=torch.uint8, device=dy.device)
    full = _unpooled(L, dy, idx, H, W)
    for mask in (src, None):
        mp = mask.data_ptr() if mask is not None else None
        ref = torch.full((N, C, H, W), 7.0, device=dy.device)
        assert L.clhip_conv3x3_bs_bwd_data(full.data_ptr(), None, w.data_ptr(), mp, ref.data_ptr(), N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
        dx = torch.full((N, C, H, W), 9.0, device=dy.device)
        assert L.clhip_conv3x3_bs_bwd_data(dy.data_ptr(), idx.data_ptr(), w.data_ptr(), mp, dx.data_ptr(), N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(dx, ref) and bool(dx.any())


def test_bs_refuses_a_16_channel_gradient():
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    assert not bs_dispatch.bs_ok(16, 64, 32, 32)
    t = torch.zeros(1 << 16, device="cuda:0")
    assert L.clhip_conv3x3_bs_bwd_data(t.data_ptr(), None, t.data_ptr(), None, t.data_ptr(), 3, 64, 16, 32, 32, t.data_ptr(), t.numel() * 4, None) == -3


def test_bs_two_geometry_launch_and_riders():
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    K = C = 64
    H = W = 32
    N = min(n for n in range(1, 200) if bs_dispatch.mixed_split(n, C, H, W) is not None)
    assert N == 97 and bs_dispatch.mixed_split(N, C, H, W) == 96          # 96 images as 32 x 4 tiles, the last one as 32 x 2 tiles
    dy, idx, w, src = _inputs(N, K, C, H, W, 41)
    ws = torch.empty(L.clhip_conv3x3_bs_ws(C, K), dtype=torch.uint8, device=dy.device)
    full = _unpooled(L, dy, idx, H, W)
    ref = torch.full((N, C, H, W), 7.0, device=dy.device)
    assert L.clhip_conv3x3_bs_bwd_data(full.data_ptr(), None, w.data_ptr(), src.data_ptr(), ref.data_ptr(), N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
    dx = torch.full((N, C, H, W), 9.0, device=dy.device)
    assert L.clhip_conv3x3_bs_bwd_data(dy.data_ptr(), idx.data_ptr(), w.data_ptr(), src.data_ptr(), dx.data_ptr(), N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, ref) and bool(dx.any())
    # the same launch with rider blocks in front: one small slab job
    jk, jc, splits = 16, 8, 5
    slabs = torch.randn((splits, 9 * jk * jc + jk), generator=torch.Generator().manual_seed(42)).to(dy.device)
    dw, db = torch.full((jk, jc, 9), 7.0, device=dy.device), torch.full((jk,), 7.0, device=dy.device)
    rdw, rdb = torch.full_like(dw, 5.0), torch.full_like(db, 5.0)
    jobs = (_lib.ReduceJob * 1)()
    jobs[0].slabs, jobs[0].dw, jobs[0].db = slabs.data_ptr(), dw.data_ptr(), db.data_ptr()
    jobs[0].K, jobs[0].C, jobs[0].splits, jobs[0].taps = jk, jc, splits, 9
    dxr = torch.full((N, C, H, W), 9.0, device=dy.device)
    assert L.clhip_conv3x3_bs_bwd_data_riders(dy.data_ptr(), idx.data_ptr(), w.data_ptr(), src.data_ptr(), dxr.data_ptr(), N, C, K, H, W, ws.data_ptr(),
                                              ws.numel(), jobs, 1, 1, 8, None) == 0
    assert L.clhip_conv3x3_bwd_weight_reduce(slabs.data_ptr(), rdw.data_ptr(), rdb.data_ptr(), jk, jc, splits, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dxr, ref)
    assert torch.equal(dw, rdw) and torch.equal(db, rdb)


W16G_SHAPES = [(3, 16, 32, 16, 16), (3, 24, 32, 16, 16), (3, 16, 32, 32, 32), (3, 24, 32, 32, 32), (161, 16, 256, 8, 8), (161, 24, 256, 8, 8)]


@pytest.mark.parametrize("shape", W16G_SHAPES, ids=lambda s: "n%d_k%d_c%d_%dx%d" % s)
def test_wino16g_unpooling_equals_two_steps(shape):
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    N, K, C, H, W = shape
    dy, idx, w, src = _inputs(N, K, C, H, W, 43)
    ws = torch.empty(L.clhip_conv3x3_wino_ws(C, K), dtype=torch.uint8, device=dy.device)
    full = _unpooled(L, dy, idx, H, W)
    for mask in (src, None):
        mp = mask.data_ptr() if mask is not None else None
        ref = torch.full((N, C, H, W), 7.0, device=dy.device)
        assert L.clhip_conv3x3_wino_bwd_data(full.data_ptr(), None, w.data_ptr(), mp, ref.data_ptr(), N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
        dx = torch.full((N, C, H, W), 9.0, device=dy.device)
        assert L.clhip_conv3x3_wino_bwd_data(dy.data_ptr(), idx.data_ptr(), w.data_ptr(), mp, dx.data_ptr(), N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(dx, ref) and bool(dx.any())


@pytest.mark.parametrize("shape", [(3, 64, 64, 16, 16), (129, 64, 128, 8, 8)], ids=lambda s: "n%d_k%d_c%d_%dx%d" % s)
def test_merged_backward_unpooling_equals_two_steps(shape):
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    N, K, C, H, W = shape
    dy, idx, w, src = _inputs(N, K, C, H, W, 44)
    x = torch.randn((N, C, H, W), generator=torch.Generator().manual_seed(45)).to(dy.device)
    nb = L.clhip_conv3x3_wino_bwd_ws(N, C, K, H, W)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dy.device)
    full = _unpooled(L, dy, idx, H, W)

    def run(g, codes, fill):
        dx = torch.full((N, C, H, W), fill, device=dy.device)
        dw, db = torch.full((K, C, 3, 3), fill, device=dy.device), torch.full((K,), fill, device=dy.device)
        assert L.clhip_conv3x3_wino_bwd(x.data_ptr(), g.data_ptr(), codes, w.data_ptr(), src.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                        N, C, K, H, W, ws.data_ptr(), ws.numel(), None) == 0
        torch.cuda.synchronize()
        return dx, dw, db
    ref = run(full, None, 7.0)
    got = run(dy, idx.data_ptr(), 9.0)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and bool(a.any())


W16_SHAPES = [(3, 16, 32, 8, 8), (129, 16, 128, 8, 8)]


@pytest.mark.parametrize("shape", W16_SHAPES, ids=lambda s: "n%d_k%d_c%d_%dx%d" % s)
def test_wino16_unpooling_equals_two_steps(shape):
    test_wino16g_unpooling_equals_two_steps(shape)


def test_merged_backward_small_batch_8x8_equals_two_steps():
    test_merged_backward_unpooling_equals_two_steps((3, 64, 64, 8, 8))


# ---------------------------------------------------------------------------------------------------- plain 8 x 8 staging
GOLDEN_PLAIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unpool_once_plain8x8.json")
# (kind, N, C, K): the layer's channels; forward C -> K, backward-data K -> C.  KT2 = 1 (N * ceil(out channels / 32) <= 512) and 2
PLAIN_CASES = [("fwd", 3, 16, 32), ("fwd", 129, 16, 128), ("bwd", 3, 32, 16), ("bwd", 129, 128, 16)]


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def plain_case(kind, N, C, K, shift=0):
    """{name: digest} of the seeded inputs and of the output of one plain 8 x 8 launch (also what records the golden file).  Inputs from
    numpy's RandomState, whose stream is frozen across numpy versions.  shift: the kernel's input tensor starts that many floats
    behind a 16-byte boundary (the float4 loads of the staging need 4-byte alignment only)."""
    import numpy as np
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    g = np.random.RandomState(46)
    x = torch.from_numpy(g.standard_normal((N, C, 8, 8)).astype(np.float32))
    dy = torch.from_numpy(g.standard_normal((N, K, 8, 8)).astype(np.float32))
    w = torch.from_numpy((g.standard_normal((K, C, 3, 3)) * 0.05).astype(np.float32))
    b = torch.from_numpy(g.standard_normal((K,)).astype(np.float32))
    out = {"x": _digest(x), "dy": _digest(dy), "w": _digest(w), "b": _digest(b)}

    def put(t):
        flat = torch.zeros(t.numel() + 4, device=dev)
        assert flat.data_ptr() % 16 == 0
        v = flat[shift:shift + t.numel()].view(t.shape)
        v.copy_(t)
        return v
    x, dy, w, b = put(x) if kind == "fwd" else x.to(dev), put(dy) if kind == "bwd" else dy.to(dev), w.to(dev), b.to(dev)
    ws = torch.empty(L.clhip_conv3x3_wino_ws(C, K), dtype=torch.uint8, device=dev)
    if kind == "fwd":
        y = torch.full((N, K, 8, 8), 9.0, device=dev)
        assert L.clhip_conv3x3_wino_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), None, N, C, K, 8, 8, 1, ws.data_ptr(), ws.numel(), None) == 0
    else:
        y = torch.full((N, C, 8, 8), 9.0, device=dev)
        assert L.clhip_conv3x3_wino_bwd_data(dy.data_ptr(), None, w.data_ptr(), x.data_ptr(), y.data_ptr(), N, C, K, 8, 8, ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert bool(y.any()) and bool(torch.isfinite(y).all())
    out["out"] = _digest(y)
    return out


@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: "%s_n%d_c%d_k%d" % c)
def test_plain_8x8_equals_the_recorded_parent_values(case):
    want = json.load(open(GOLDEN_PLAIN))["%s_n%d_c%d_k%d" % case]
    got = plain_case(*case)
    for name in ("x", "dy", "w", "b"):
        assert got[name] == want[name], "the seeded input %s differs from the recorded one: the generator changed, not the kernel" % name
    assert got["out"] == want["out"]
    assert plain_case(*case, shift=1)["out"] == want["out"]           # the input tensor one float behind a 16-byte boundary
