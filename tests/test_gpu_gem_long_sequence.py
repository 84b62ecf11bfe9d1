"""GEM on a sequence of more than 16 tasks: test_gpu_parity.py::test_gem_observe_device_qp_equals_host_path taken to 18 tasks.
From the 17th task on a Gram matrix has more than 16 rows and GemNet calls the wide entries of csrc/gem_wide.hip
(clhip_gem_gram_wide -> clhip_gem_qp_wide -> clhip_gem_project_dev_wide; with an injected host solver clhip_gem_gram_wide ->
host QP -> clhip_gem_project_wide).  Before those entries existed this run raised in the first observe of the 17th task
("clhip_gem_gram failed": m = 17 > 16)."""
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

N_TASKS, NC, N_MEM, BATCH = 18, 2, 4, 4
LR = 1e-4      # margin 0.5 adds half of every memory gradient (17 at the end) to the step: the 1e-2 of the 3-task test diverges by task 12


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def run_sequence(on_device):
    from clsurvey_amd import _lib, models
    from clsurvey_amd.methods.gem import GemNet, extend_head
    from oracle import qp_ref
    L = _lib.lib()
    torch.manual_seed(4)
    m = extend_head(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), NC), NC * N_TASKS)
    gem = GemNet(m, NC * N_TASKS, N_TASKS, [NC] * N_TASKS, N_MEM, LR, 0.0, 0.5, batch_size=BATCH, in_shape=(3, 32, 32), device=dev())
    gem.host_qp = None if on_device else qp_ref.project2cone2_coefficients     # the host cross-check path is injected
    gen = torch.Generator().manual_seed(9)
    counts = []
    for t in range(N_TASKS):
        if t == 16:
            # the 17th task starts from a pickled wrapper: the transient buffers are rebuilt at the sizes of an 18-task sequence
            buf = io.BytesIO()
            torch.save(gem, buf)
            buf.seek(0)
            gem = torch.load(buf, weights_only=False)
            gem.init_setup(lr=LR, weight_decay=0.0, memory_strength=0.5)
            gem.host_qp = None if on_device else qp_ref.project2cone2_coefficients
            assert gem.n_tasks == N_TASKS and gem.observed_tasks == list(range(16))
            assert gem._gram.numel() == N_TASKS * N_TASKS and gem._v.numel() == N_TASKS
            assert gem._gram_ws.numel() == max(L.clhip_gem_gram_ws(16), L.clhip_gem_gram_wide_ws(N_TASKS))
            assert gem.G.shape == (N_TASKS, gem.A.numel)
        for _ in range(2):
            x = torch.randn(BATCH, 3, 32, 32, generator=gen).to(dev())
            y = (torch.randint(0, NC, (BATCH,), generator=gen) + NC * t).to(dev())
            _, _, st = gem.observe(x, t, y)
            counts.append((t, int(st["projected_grads"][0])))
    gem.check_qp_status()
    return [p.detach().clone() for p in gem.net.parameters()], counts


def test_gem_observe_18_tasks_device_qp_equals_host_path():
    """18 tasks of 2 classes, n_memories = batch = 4, two observe calls per task, margin 0.5: the device path and the injected
    oracle/qp_ref.py path project in the same steps, by the same counts of violated constraints, and end with bitwise equal
    parameters (the coefficients are rounded to fp32 at the same place); at least one projection runs with 17 memory rows."""
    (p_dev, c_dev), (p_host, c_host) = run_sequence(True), run_sequence(False)
    print("MEASURED|gem_18_tasks|projected constraints per observe (task, count)|%s" % (c_dev,))
    assert c_dev == c_host, (c_dev, c_host)
    assert any(c > 0 for t, c in c_dev if t >= 17), c_dev
    assert any(c > 0 for t, c in c_dev if t == 16), c_dev
    for a, b in zip(p_dev, p_host):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_gem_refuses_more_than_64_tasks():
    """The limit is reported at construction, not by a kernel entry in the first observe of task 65."""
    from clsurvey_amd import models
    from clsurvey_amd.methods.gem import GemNet, extend_head
    m = extend_head(models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 1), 65)
    with pytest.raises(ValueError, match="64"):
        GemNet(m, 65, 65, [1] * 65, 1, 1e-2, 0.0, 0.5, batch_size=2, in_shape=(3, 32, 32), device=dev())
