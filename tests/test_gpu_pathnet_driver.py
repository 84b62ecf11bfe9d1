"""PathNet end to end on the GPU: --method_name pathnet through the two-phase driver on two tiny synthetic tasks with
--test (phase-1 search per LR, tournament, evaluation over bestPath[task] with the task's saved head)."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pathnet_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

COMMON = ["small_VGG9_cl_128_128", "--lr_grid", "1e-1,3e-2", "--num_epochs", "16", "--batch_size", "40", "--saving_freq", "100",
          "--decaying_factor", "1", "--max_attempts_per_task", "1"]


def test_pathnet_through_driver(tmp_path):
    from clsurvey_amd import models
    from clsurvey_amd.framework import driver, inference
    from clsurvey_amd.framework.tasks import SyntheticTaskSequence
    from clsurvey_amd.methods import method as M
    root = str(tmp_path)
    ds = SyntheticTaskSequence(os.path.join(root, "data"), task_count=2, classes_per_task=4, sizes=(160, 40, 40), hw=32,
                               noise=0.4, name="tiny2")
    torch.manual_seed(0)
    np.random.seed(0)
    raw = models.parse_model_name("small_VGG9_cl_128_128", (32, 32), 4)
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    torch.save(raw, os.path.join(root, "models", "small_VGG9_cl_128_128.pth.tar"))
    pn = M.parse("pathnet")
    pn.hyperparams["N"] = 2
    pn.static_hyperparams["M"], pn.static_hyperparams["generations"] = 4, 2       # 8 epochs per participant per generation
    out = driver.main(COMMON + ["--method_name", "pathnet", "--results_root", root, "--test"], method=pn, dataset=ds)
    res = out["results"]
    assert sorted(res) == [0, 1]
    print("pathnet through the driver:", {i: res[i]["seq_res"] for i in res})
    acc_t1 = res[0]["seq_res"][0]
    assert len(acc_t1) == 2 and acc_t1[0] == acc_t1[1], acc_t1                   # task 1 is not forgotten, to the last sample
    assert all(0.0 <= a <= 100.0 for i in res for a in res[i]["seq_res"][i]), res
    m1, m2 = (torch.load(p, weights_only=False) for p in out["model_paths"])
    # N is 2 for task 1; where task 1 misses the framework's threshold the driver grows it to 3 for task 2 (decay_operator)
    assert m1.N == 2 and m2.N in (2, 3) and m1.bestPath.shape == (2, 8, 2) and m2.bestPath.shape == (2, 8, m2.N)
    assert (m1.bestPath[0] >= 0).all() and (m1.bestPath[1] == -1).all()
    assert (m2.bestPath[0][:, :2] == m1.bestPath[0]).all() and (m2.bestPath[0][:, 2:] == -1).all() and (m2.bestPath[1] >= 0).all()
    p1, p2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    groups = ["convs.%d" % i for i in range(6)] + ["fcs.%d" % i for i in range(2)]
    frozen, changed = 0, 0
    for l, g in enumerate(groups):
        for mod in range(4):
            for w in ("weight", "bias"):
                n = "%s.%d.%s" % (g, mod, w)
                same = torch.equal(p1[n].detach().cpu(), p2[n].detach().cpu())
                if mod in m1.bestPath[0][l]:
                    assert same, "a module of task 1's best path moved while task 2 trained: " + n
                    frozen += 1
                else:
                    changed += not same
    assert frozen == 8 * 2 * 2 and changed > 0
    for n, p in m2.initial_model.named_parameters():
        assert torch.equal(p.detach().cpu(), dict(m1.initial_model.named_parameters())[n].detach().cpu())
    # best_model.pth.tar of task 1 reloads and evaluates to the number the driver reported
    again = inference.test_model(pn, torch.load(out["model_paths"][0], weights_only=False), ds.get_task_dataset_path(task_name="1"),
                                 0, target_head=inference.get_prev_heads(out["model_paths"][0], "0"), batch_size=40, subset="test",
                                 task_idx=0)
    assert again == acc_t1[0]
    # the evaluation strategy (head swapped in, forward over bestPath[task]) against vgg_pathnet.Net.forward restated on CPU
    state = {n: p.detach().cpu() for n, p in m2.named_parameters() if not n.startswith("initial_model.")}
    x = torch.randn(40, 3, 32, 32, generator=torch.Generator().manual_seed(5))
    for task in (0, 1):
        holder = SimpleNamespace(model=m2, heads=[copy.deepcopy(m2.classifier[0])], current_head_idx=0, batch_size=40, task_idx=task)
        got = pn.get_output(x.cuda(), holder)
        with torch.no_grad():
            want = PR.direct_forward(state, x, m2.bestPath[task], m2.N, m2.maxpool_idxs)
        assert PR.rel(got, want) <= PR.TOL_LOGITS, (task, PR.rel(got, want))
    for t in (1, 2):
        tdir = os.path.join(out["manager"].parent_exp_dir, "task_%d" % t, "TASK_TRAINING")
        assert os.path.exists(os.path.join(tdir, "best_model.pth.tar")) and os.path.exists(os.path.join(tdir, "SUCCESS.FLAG"))
