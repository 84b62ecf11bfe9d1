"""Host logic of the PathNet trainers without a GPU: `Tournament` and `Phase1` (methods/pathnet_main.py) over a scripted
stand-in for the device reproduce, event by event, what the reference's Appr.train did over the same scripted validation
accuracies under the same np.random.seed (fixture G39, tests/golden/make_g39.py); and the `pathnet` method row."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import g38_common as G  # noqa: E402
import g39_common as S  # noqa: E402


@pytest.fixture(scope="module")
def g39():
    with open(os.path.join(HERE, "golden", "G39_pathnet_trainer.json")) as f:
        return json.load(f)


def make_net():
    from clsurvey_amd import models
    from clsurvey_amd.methods import pathnet as PN
    raw = models.VGGSlim(cfg=G.CFG, num_classes=G.NCLS, classifier_inputdim=64 * 2 * 2, classifier_dim1=G.FC[0],
                         classifier_dim2=G.FC[1])
    return PN.PathNet(raw, (3, G.HW, G.HW), [(t, G.NCLS) for t in range(G.NTASKS)], [S.N, S.M])


class Scripted:
    """The device interface of the trainers: an epoch advances a counter (the 'model state'), validation accuracies come
    from the table; every call is logged in the fixture's format."""

    def __init__(self, net, val_acc):
        self.net, self.acc, self.events, self.ticks, self.made = net, iter(val_acc), [], 0.0, 0

    def _own(self):
        return [(n, p) for n, p in self.net.named_parameters() if not n.startswith("initial_model.")]

    def reinit_modules(self, t):
        from clsurvey_amd.methods import pathnet_main as PM
        with torch.no_grad():
            for _, p in self._own():
                p.add_(1.0)
        PM.reinit_modules(self.net, t)
        init = dict(self.net.initial_model.named_parameters())
        self.events.append(["reinit", t, sorted(n for n, p in self._own() if torch.equal(p, init[n]))])

    def unfreeze(self, t, path):
        train = self.net.trainable_modules(t, path)
        kinds = ["convs.%d" % i for i in range(len(self.net.convs))] + ["fcs.%d" % i for i in range(len(self.net.fcs))]
        names = sorted("%s.%d.%s" % (k, m, w) for k, mods in zip(kinds, train) for m in mods for w in ("weight", "bias"))
        self.events.append(["unfreeze", np.asarray(path).tolist(), names])

    def new_optimizer(self, lr):
        self.events.append(["optim", lr])
        self.made += 1
        return {"ordinal": self.made - 1, "lr": lr}

    def set_lr(self, opt, lr):
        self.events.append(["set_lr", opt["ordinal"], lr])
        opt["lr"] = lr

    def train_epoch(self, t, path, opt):
        self.ticks += 1
        self.events.append(["train", opt["ordinal"], opt["lr"]])

    def eval(self, t, split, path):
        self.events.append(["eval", split])
        return (1.0, next(self.acc)) if split == "val" else (1.0, 0.0)

    def snapshot(self):
        self.events.append(["save", self.ticks])
        return self.ticks

    def restore(self, state):
        self.events.append(["restore", state])
        self.ticks = state


def policy_events(rec):
    return [e for e in rec["events"] if e[0] != "torch.save"]        # the files are written by train_task, not by the policy


def test_tournament_reproduces_the_reference_trace(g39):
    from clsurvey_amd.methods import pathnet_main as PM
    net = make_net()
    kept = 0
    for t in (0, 1):
        rec = g39["joint_t%d" % t]
        dev = Scripted(net, rec["val_acc"])
        dev.ticks = 0.0 if t == 0 else g39["joint_t0"]["ticks"]
        np.random.seed(S.SEEDS["joint_t%d" % t])
        paths, winner, best = PM.Tournament(dev, S.N, S.M, net.L, S.GENERATIONS, S.NEPOCHS, S.LR, S.LR_FACTOR, S.LR_PATIENCE,
                                            log=lambda *_: None).run(t)
        net.bestPath[t] = paths[winner]
        assert dev.events == policy_events(rec)
        assert best == rec["best_acc"] and net.bestPath.tolist() == rec["bestPath"] and dev.ticks == rec["ticks"]
        assert np.random.rand() == rec["rng_after"]                  # the same number of draws, in the same order
        ev = [e for e in dev.events if e[0] in ("optim", "train", "unfreeze")]
        kept += sum(1 for a, b in zip(ev, ev[1:]) if a[0] == "unfreeze" and b[0] == "train")
    print("generations in which a winner kept its optimizer:", kept)


def test_phase1_reproduces_the_reference_trace(g39):
    from clsurvey_amd.methods import pathnet_main as PM
    net = make_net()
    for t in (0, 1):
        rec = g39["phase1_t%d" % t]
        if t == 1:
            net.bestPath[0] = np.array(g39["joint_t0"]["bestPath"][0])
        dev = Scripted(net, rec["val_acc"])
        dev.ticks = 0.0 if t == 0 else g39["phase1_t0"]["ticks"]
        np.random.seed(S.SEEDS["phase1_t%d" % t])
        state, best = PM.Phase1(dev, S.M, net.L, S.PHASE1_EPOCHS, S.LR, S.LR_FACTOR, S.LR_PATIENCE, log=lambda *_: None).run(t)
        assert dev.events == policy_events(rec)
        assert best == rec["best_acc"] and dev.ticks == rec["ticks"] and np.random.rand() == rec["rng_after"]
        assert (state is not None) == (rec["returns"] == "OrderedDict")
        assert net.bestPath.tolist() == rec["bestPath"]                 # the search leaves the best paths alone
        unfreeze = [e for e in dev.events if e[0] == "unfreeze"][0]
        assert unfreeze[1] == [list(range(S.M))] * net.L                # every module listed


def test_method_row_matches_the_reference(g39):
    from clsurvey_amd.methods import method as M
    ref = g39["method"]
    m = M.parse("pathnet")
    pairs = lambda d: [[str(k), v] for k, v in d.items()] if d is not None else None      # noqa: E731
    assert type(m).__name__ == ref["class"] == "Pathnet"
    assert (m.name, m.eval_name, m.extra_hyperparams_count) == (ref["name"], ref["eval_name"], ref["extra_hyperparams_count"])
    assert m.category.name == ref["category"] == "MASK_BASED"
    assert pairs(m.hyperparams) == ref["hyperparams"] and pairs(m.static_hyperparams) == ref["static_hyperparams"]
    assert ref["instance_attrs"] == {}
    for hook in ref["hooks"]:
        assert callable(getattr(m, hook, None)), hook
    for flag in ("start_scratch", "wrap_first_task_model", "no_framework", "grid_chkpt"):
        assert bool(getattr(m, flag, False)) == bool(ref["flags"].get(flag, False)), flag
    for a, want in ref["decay_operator"]:
        got = m.decay_operator(a, 1)
        assert got == want and isinstance(got, int)
    with pytest.raises(AssertionError):
        m.decay_operator(3, 0.5)
    assert m.spec["output"] == "pathnet" and m.spec["evaluate"] == "swap_head"


def test_hat_main_still_refuses_pathnet_and_pathnet_main_refuses_the_rest():
    from clsurvey_amd.methods import hat_main, pathnet_main
    with pytest.raises(NotImplementedError):
        hat_main.main({"approach": "pathnet", "task_count": 1})
    with pytest.raises(NotImplementedError):
        pathnet_main.main({"approach": "hat", "task_count": 1})
    with pytest.raises(NotImplementedError, match="alexnet"):
        pathnet_main.main({"approach": "pathnet", "task_count": 1, "model_name": "alexnet_pretrained"})
