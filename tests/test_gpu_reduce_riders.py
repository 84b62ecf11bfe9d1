"""CLHIP_REDUCE_RIDERS: the weight-gradient slabs that are complete when the lowest bf16-split backward-data launch of a pass goes
out are reduced by rider blocks of that launch (csrc/bsconv.hip, bs_conv_riders_kernel) instead of by the reduction launch at the end
of the pass.  A rider runs the reduction launch's own block code (csrc/wgrad_reduce.hpp) and the convolution blocks run the plain
launch's body with the block index they have there, so every result must be BITWISE equal between the settings of the switch:
0 = the reduction launch alone, 1 / 2 / 3 = riders in front of / behind / spread through the convolution blocks.  The library reads
the switch once, so every setting computes all cases of an environment in one child process of its own (this file run as a script)
and the tests compare the saved tensors.  The 16-wide host geometry exists only where the bf16-split path takes a 16 x 16 map:
its case runs under CLHIP_BS=2."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TINY_CFG = [64, "M", 64, "M"]
# case -> (model name or cfg, input height = width, batch)
CASES = {
    "small_n3": ("small_VGG9_cl_128_128", 64, 3),          # ragged last tile groups
    "small_n8": ("small_VGG9_cl_128_128", 64, 8),
    "small_n100": ("small_VGG9_cl_128_128", 64, 100),      # layer 2's backward-data is the two-geometry launch: 768 + 32 blocks, NA = 96
    "base_n4": ("base_VGG9_cl_512_512", 64, 4),            # other channel counts, more jobs
    "tiny16": (TINY_CFG, 32, 8),                           # two conv layers: the smallest deferred reduction; host on a 16 x 16 map
    "in32": ("small_VGG9_cl_128_128", 32, 8),              # declines: no layer above the first keeps the bf16-split backward-data
}
# environment -> (its variables, the settings of the switch compared, the cases computed under it)
GROUPS = {
    "default": ({}, ("0", "1", "2", "3"), ["small_n3", "small_n8", "small_n100", "base_n4", "in32"]),
    "bs2": ({"CLHIP_BS": "2"}, ("0", "1", "2", "3"), ["tiny16"]),
    "nobs": ({"CLHIP_BS": "0"}, ("0", "1"), ["small_n8"]),                       # declines: no bf16-split host
    "overlap": ({"CLHIP_WGRAD_OVERLAP": "1"}, ("0", "1"), ["small_n8"]),         # declines: side-stream slabs, immediate reductions
}


def _compute(case):
    import torch
    from clsurvey_amd import models, net
    name, hw, n = CASES[case]
    dev = torch.device("cuda:0")
    torch.manual_seed(30)
    if isinstance(name, str):
        m = models.parse_model_name(name, (hw, hw), 20)
    else:
        m = models.VGGSlim(cfg=name, num_classes=20, classifier_inputdim=64 * (hw // 4) ** 2)
    eng = net.NetEngine(m, n, (3, hw, hw), dev)
    eng.ws.zero_()                 # (padding the kernels never write must not differ between two processes)
    g = torch.Generator().manual_seed(31)
    x = torch.randn((n, 3, hw, hw), generator=g).to(dev)
    y = torch.randint(0, 20, (n,), generator=g).to(dev)
    out = {}
    for kind in ("ce_mean", "ce_sum"):
        eng.arena.grad.zero_()
        loss, _ = eng.loss_step(x, y, kind, True)
        torch.cuda.synchronize()
        out[kind + "/loss"] = loss.cpu().clone()
        out[kind + "/grad"] = eng.arena.grad.cpu().clone()
        for layer in (1, 2):
            out["%s/input%d" % (kind, layer)] = eng.layer_input(layer, n).cpu().clone()
    out["rider_passes"] = torch.tensor(eng.reduce_rider_count())
    return out


def _child(group, path):
    import torch
    torch.save({case: _compute(case) for case in GROUPS[group][2]}, path)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{(group, setting): {case: {name: tensor}}} — one child process per environment and setting of the switch, six at a time."""
    import torch
    d = tmp_path_factory.mktemp("reduce_riders")
    todo = [(group, setting) for group, (_, settings, _) in GROUPS.items() for setting in settings]
    res = {}
    for lo in range(0, len(todo), 6):
        running = []
        for group, setting in todo[lo:lo + 6]:
            path = str(d / ("%s_%s.pt" % (group, setting)))
            env = dict(os.environ, CLHIP_REDUCE_RIDERS=setting, **GROUPS[group][0])
            env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
            running.append((group, setting, path, subprocess.Popen([sys.executable, os.path.abspath(__file__), group, path], env=env, cwd=ROOT,
                                                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        failed = []
        for group, setting, path, proc in running:
            text, _ = proc.communicate(timeout=600)
            if proc.returncode != 0:
                failed.append((group, setting, proc.returncode, text[-2500:]))
            else:
                res[(group, setting)] = torch.load(path)
        assert not failed, failed
    return res


def _same(results, group, case, rider_passes):
    """rider_passes: backward passes of the case whose host launch must have carried riders with the switch on (0: the plan or the
    launch declines and the bitwise equality below is that of the fallback); with the switch off none may."""
    import torch
    ref = dict(results[(group, "0")][case])
    assert int(ref.pop("rider_passes")) == 0
    assert bool(ref["ce_mean/grad"].any()) and bool(ref["ce_sum/grad"].any())
    for setting in GROUPS[group][1][1:]:
        got = dict(results[(group, setting)][case])
        assert int(got.pop("rider_passes")) == rider_passes, (case, setting)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert ref[k].dtype == got[k].dtype and torch.equal(ref[k], got[k]), "%s %s: CLHIP_REDUCE_RIDERS=%s differs from 0" % (case, k, setting)


@pytest.mark.parametrize("case", ["small_n3", "small_n8", "small_n100", "base_n4"])
def test_vgg9_passes(results, case):
    _same(results, "default", case, 2)


def test_smallest_deferred_reduction_16_wide_host(results):
    _same(results, "bs2", "tiny16", 2)


def test_declines_without_bf16_split_host(results):
    _same(results, "nobs", "small_n8", 0)


def test_declines_side_stream_weight_gradients(results):
    _same(results, "overlap", "small_n8", 0)


def test_declines_layers_off_their_paths(results):
    _same(results, "default", "in32", 0)


# ---------------------------------------------------------------------------------------------------- kernel level
# (K, C, splits, taps) of the synthetic slab jobs: every split count around the 16 split-lanes of a reduction block (one lane busy,
# one idle, all with one split, the first with two, three rounds), a slab whose length is no multiple of 4 (scalar loads, a
# ragged last unit), 25 taps
JOBS = [(16, 8, 1, 9), (16, 8, 15, 9), (16, 16, 16, 9), (32, 8, 17, 9), (16, 8, 33, 9), (3, 5, 7, 9), (8, 4, 5, 25)]
# (N, C, K, H = W, un-pooling, place, riders): the three host geometries.  Few riders: every rider loops over many of the 147 units;
# 24 riders spread through 64 convolution blocks: 11 groups of 8, every third a rider group, two convolution groups behind the
# last one; more riders than units: clamped to 152, and too many to spread through 64 convolution blocks (they go behind them)
HOSTS = [(3, 64, 64, 32, True, 2, 8), (32, 64, 64, 16, False, 3, 24), (4, 64, 64, 8, False, 1, 256), (8, 64, 64, 32, False, 3, 1024)]


def _two_level(slabs, K, C, taps):
    """wgrad_reduce_block's order in f64 on the CPU: lane j sums splits [j q, (j + 1) q) in order, the 16 lane sums are added in order."""
    import torch
    s = slabs.double()
    q = (s.shape[0] + 15) // 16
    tot = torch.zeros(s.shape[1], dtype=torch.float64)
    for j in range(16):
        lane = torch.zeros(s.shape[1], dtype=torch.float64)
        for sp in range(j * q, min(s.shape[0], (j + 1) * q)):
            lane = lane + s[sp]
        tot = tot + lane
    f = tot.float()
    return f[:taps * K * C].view(taps, K, C).permute(1, 2, 0).contiguous(), f[taps * K * C:].clone()


@pytest.mark.parametrize("host", HOSTS, ids=lambda h: "n%d_hw%d_%s_place%d_r%d" % (h[0], h[3], "unpool" if h[4] else "plain", h[5], h[6]))
def test_host_launch_with_synthetic_jobs(host):
    import ctypes as C
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    N, Cc, K, hw, unpool, place, riders = host
    g = torch.Generator().manual_seed(32)
    dy = torch.randn((N, K, hw // 2, hw // 2) if unpool else (N, K, hw, hw), generator=g).to(dev)
    idx = torch.randint(0, 5, (N, K, hw // 2, hw // 2), generator=g).to(torch.uint8).to(dev) if unpool else None
    w = (torch.randn((K, Cc, 3, 3), generator=g) * 0.05).to(dev)
    src = torch.randn((N, Cc, hw, hw), generator=g).to(dev)
    ws = torch.empty(L.clhip_conv3x3_bs_ws(Cc, K), dtype=torch.uint8, device=dev)
    ip = idx.data_ptr() if unpool else None
    dx_ref = torch.full((N, Cc, hw, hw), 7.0, device=dev)
    assert L.clhip_conv3x3_bs_bwd_data(dy.data_ptr(), ip, w.data_ptr(), src.data_ptr(), dx_ref.data_ptr(), N, Cc, K, hw, hw, ws.data_ptr(),
                                       ws.numel(), None) == 0
    jobs = (_lib.ReduceJob * len(JOBS))()
    keep = []
    for j, (jk, jc, splits, taps) in enumerate(JOBS):
        total = taps * jk * jc + jk
        slabs = torch.randn((splits, total), generator=g).to(dev)
        dw = torch.full((jk, jc, taps), 7.0, device=dev)
        db = torch.full((jk,), 7.0, device=dev)
        keep.append((slabs, dw, db))
        jobs[j].slabs, jobs[j].dw, jobs[j].db = slabs.data_ptr(), dw.data_ptr(), db.data_ptr()
        jobs[j].K, jobs[j].C, jobs[j].splits, jobs[j].taps = jk, jc, splits, taps
    dx = torch.full((N, Cc, hw, hw), 9.0, device=dev)
    assert L.clhip_conv3x3_bs_bwd_data_riders(dy.data_ptr(), ip, w.data_ptr(), src.data_ptr(), dx.data_ptr(), N, Cc, K, hw, hw, ws.data_ptr(),
                                              ws.numel(), jobs, len(JOBS), place, riders, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref) and bool(dx.any())
    for (jk, jc, splits, taps), (slabs, dw, db) in zip(JOBS, keep):
        cpu_dw, cpu_db = _two_level(slabs.cpu(), jk, jc, taps)
        assert torch.equal(dw.cpu(), cpu_dw) and torch.equal(db.cpu(), cpu_db), (jk, jc, splits, taps)
        if taps == 9:
            rdw, rdb = torch.full_like(dw, 5.0), torch.full_like(db, 5.0)
            assert L.clhip_conv3x3_bwd_weight_reduce(slabs.data_ptr(), rdw.data_ptr(), rdb.data_ptr(), jk, jc, splits, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(dw, rdw) and torch.equal(db, rdb), (jk, jc, splits)


def test_refusals_launch_nothing():
    import torch
    from clsurvey_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    t = torch.zeros(1 << 20, device=dev)
    ws = torch.empty(L.clhip_conv3x3_bs_ws(64, 64), dtype=torch.uint8, device=dev)
    jobs = (_lib.ReduceJob * 33)()
    for j in jobs:
        j.slabs, j.dw, j.db, j.K, j.C, j.splits, j.taps = t.data_ptr(), t.data_ptr(), None, 4, 4, 2, 9

    def call(n_jobs, place, riders):
        return L.clhip_conv3x3_bs_bwd_data_riders(t.data_ptr(), None, t.data_ptr(), None, t.data_ptr(), 1, 64, 64, 8, 8, ws.data_ptr(), ws.numel(),
                                                  jobs, n_jobs, place, riders, None)
    for bad in ((0, 1, 8), (33, 1, 8), (1, 0, 8), (1, 4, 8), (1, 1, 0), (1, 1, 12), (1, 1, -8)):
        assert call(*bad) == -3, bad
    jobs[0].splits = 0
    assert call(1, 1, 8) == -1
    torch.cuda.synchronize()
    assert not bool(t.any())


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
