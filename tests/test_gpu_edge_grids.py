"""CLHIP_EDGE_GRIDS: the prepared-weights jobs of a pass as blocks of the first layer's forward grid (csrc/conv3x3.hip,
c3w64_relu_pool_wt_kernel) against the launch of their own.  Both run the same device code per job and per first-layer block, so every
result must be BITWISE equal between the settings of the switch: 0 = separate launches, 1 = merged grid with the weight blocks at
the end (the default), 2 = merged grid with the weight blocks in front.  The library reads the switch once, so every setting computes all cases of
an environment in one child process of its own (this file run as a script) and the tests compare the saved tensors."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# case -> (model name, input height = width, batch, what runs)
CASES = {
    "small_n3": ("small_VGG9_cl_128_128", 64, 3, "steps"),         # odd batch: the last tile group of the deeper layers is ragged
    "small_n8": ("small_VGG9_cl_128_128", 64, 8, "steps"),
    "in32": ("small_VGG9_cl_128_128", 32, 8, "steps"),             # declines: first layer on conv3x3_c3_relu_pool_kernel
    "bn": ("small_VGG9_cl_128_128_BN", 64, 4, "steps"),            # declines: BatchNorm layers take the unfused launches
    "forward": ("small_VGG9_cl_128_128", 64, 8, "forward"),        # clhip_net_forward: no backward image set in the table
    "base_n4": ("base_VGG9_cl_512_512", 64, 4, "steps"),           # a second width: more weight jobs
}
# environment -> (its variables, the settings of the switch compared, the cases computed under it)
GROUPS = {
    "default": ({}, ("0", "1", "2"), ["small_n3", "small_n8", "in32", "bn", "forward", "base_n4"]),
    "direct": ({"CLHIP_WINO": "0", "CLHIP_BS": "0"}, ("0", "1"), ["small_n8"]),          # declines: no images to prepare
    "overlap": ({"CLHIP_WGRAD_OVERLAP": "1"}, ("0", "1"), ["small_n8"]),                 # side-stream weight gradients, immediate reductions
}


def _compute(case):
    """Every tensor the switch could touch, as CPU tensors."""
    import torch
    from clsurvey_amd import models, net
    name, hw, n, what = CASES[case]
    dev = torch.device("cuda:0")
    torch.manual_seed(20)
    m = models.parse_model_name(name, (hw, hw), 20)
    eng = net.NetEngine(m, n, (3, hw, hw), dev)
    eng.ws.zero_()                 # (padding the kernels never write must not differ between two processes)
    g = torch.Generator().manual_seed(21)
    x = torch.randn((n, 3, hw, hw), generator=g).to(dev)
    y = torch.randint(0, 20, (n,), generator=g).to(dev)
    out = {}

    def grab(tag):
        torch.cuda.synchronize()
        for layer in (1, 2):
            out["%s/input%d" % (tag, layer)] = eng.layer_input(layer, n).cpu().clone()
        for layer in (0, 1):
            try:
                out["%s/pool_idx%d" % (tag, layer)] = eng.pool_idx(layer, n).cpu().clone()
            except RuntimeError:       # (a layer without a pool)
                pass
        out["%s/prepared_weights" % tag] = eng.prepared_weights().cpu().clone()

    if what == "forward":
        out["forward/logits"] = eng.forward(x).cpu().clone()
        grab("forward")
        out["merged_launches"] = torch.tensor(eng.edge_grid_count())
        return out
    for kind in ("ce_mean", "ce_sum"):
        eng.arena.grad.zero_()
        loss, _ = eng.loss_step(x, y, kind, True)
        out[kind + "/loss"] = loss.cpu().clone()
        out[kind + "/grad"] = eng.arena.grad.cpu().clone()
        grab(kind)
    out["merged_launches"] = torch.tensor(eng.edge_grid_count())     # forward passes that took the merged grid (not compared)
    return out


def _child(group, path):
    import torch
    torch.save({case: _compute(case) for case in GROUPS[group][2]}, path)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{(group, setting): {case: {name: tensor}}} — one child process per environment and setting of the switch."""
    import torch
    d = tmp_path_factory.mktemp("edge_grids")
    res = {}
    for group, (extra, settings, _) in GROUPS.items():
        for setting in settings:
            path = str(d / ("%s_%s.pt" % (group, setting)))
            env = dict(os.environ, CLHIP_EDGE_GRIDS=setting, **extra)
            env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), group, path], env=env, capture_output=True, text=True,
                               timeout=600, cwd=ROOT)
            assert r.returncode == 0, (group, setting, r.stdout[-2500:], r.stderr[-2500:])
            res[(group, setting)] = torch.load(path)
    return res


def _same(results, group, case, merged, expect_images=None):
    """merged: forward passes of the case that must have gone out as the merged grid with the switch on (0: the shape declines, the
    bitwise equality below is that of the fallback); with the switch off none may."""
    import torch
    ref = dict(results[(group, "0")][case])
    assert int(ref.pop("merged_launches")) == 0
    assert any(k.endswith("/prepared_weights") for k in ref)
    for k, v in ref.items():
        if k.endswith("/prepared_weights") and expect_images is not None:
            assert (v.numel() > 0 and bool(v.any())) == expect_images, (case, k, v.numel())
    for setting in GROUPS[group][1][1:]:
        got = dict(results[(group, setting)][case])
        assert int(got.pop("merged_launches")) == merged, (case, setting)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert ref[k].dtype == got[k].dtype and torch.equal(ref[k], got[k]), "%s %s: CLHIP_EDGE_GRIDS=%s differs from 0" % (case, k, setting)


@pytest.mark.parametrize("case", ["small_n3", "small_n8"])
def test_headline_path_small_batch(results, case):
    _same(results, "default", case, 2, expect_images=True)
    ref = results[("default", "0")][case]
    assert bool(ref["ce_mean/grad"].any()) and "ce_sum/pool_idx0" in ref and "ce_sum/pool_idx1" in ref


def test_declines_first_layer_on_the_32_wide_kernel(results):
    _same(results, "default", "in32", 0)


def test_declines_batchnorm_model(results):
    _same(results, "default", "bn", 0)


def test_declines_without_prepared_weights(results):
    _same(results, "direct", "small_n8", 0, expect_images=False)


def test_side_stream_weight_gradients(results):
    _same(results, "overlap", "small_n8", 2)


def test_forward_only_call(results):
    _same(results, "default", "forward", 1, expect_images=True)
    assert bool(results[("default", "0")]["forward"]["forward/logits"].any())


def test_second_width(results):
    _same(results, "default", "base_n4", 2, expect_images=True)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
