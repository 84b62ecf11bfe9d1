"""PathNet trainer on the HIP path: what src/methods/HAT/run.py:main drives for approach == 'pathnet' —
approaches/pathnet.py (binary tournament over paths) and approaches/pathnet_finetune.py (phase-1 search: one participant,
every module listed) — as two small pieces of host policy over a device object:

  * `Tournament` / `Phase1` hold the reference's control flow and its NumPy random draws, in its order, and know nothing
    of the device: they call reinit_modules / unfreeze / new_optimizer / set_lr / train_epoch / eval / snapshot / restore
    on whatever they are given (tests/test_pathnet_trainer_cpu.py drives them over a scripted stand-in);
  * `PathDevice` is that object over a PathEngine: one batch = pack, the net's plan with CE, fold, clip + SGD
    (methods/pathnet.py); loss / accuracy are device counters read once per pass.

Kept as the reference has them (PathNet): unfreeze_path freezes the best path of the FIRST task only while
reinit_modules spares the best paths of ALL earlier tasks; `elif patience == 0` of the tournament compares a list and never
fires; the loser's optimizer is renewed every generation, the winner's is kept only when the winner is participant 1.
"""
import os
import time
from copy import deepcopy
from types import SimpleNamespace

import numpy as np
import torch

from ..data import DeviceLoader, load_task_datasets
from . import pathnet as PN
from .train_common import PatiencePlan

# run.py:109-110 passes lr_factor and lr_patience to every approach; clipgrad is the approaches' default (pathnet.py:15-16)
LR_FACTOR, LR_PATIENCE, CLIPGRAD = 2, 30, 1000
MOMENTUM = 0.9


class Tournament:
    """approaches/pathnet.py:101-206 for one task.  run() returns (paths [P][L][N], winner, best validation accuracy)."""

    def __init__(self, dev, N, M, L, generations, nepochs, lr, lr_factor=LR_FACTOR, lr_patience=LR_PATIENCE, P=2, log=print):
        self.dev, self.N, self.M, self.L, self.P = dev, int(N), int(M), int(L), int(P)
        self.generations = int(generations)
        self.nepochs = int(nepochs) // self.generations          # the same number of updates as a plain run (pathnet.py:40)
        self.lr, self.lr_factor, self.lr_patience = lr, lr_factor, lr_patience
        self.log = log

    def run(self, t):
        dev, P, L, N, M = self.dev, self.P, self.L, self.N, self.M
        if t > 0:
            dev.reinit_modules(t)
        Path = np.random.randint(0, M - 1, size=(P, L, N))        # overwritten below; drawn for the generator's state
        guesses = list(range(M))
        optim, lr, patience, best_acc = [], [], [], []
        for p in range(P):
            optim.append(dev.new_optimizer(self.lr))
            lr.append(self.lr)
            patience.append(self.lr_patience)
            best_acc.append(0)
            for j in range(L):
                np.random.shuffle(guesses)                        # ONE list, shuffled on
                Path[p, j, :] = guesses[:N]
        winner = 0
        best_state = dev.snapshot()
        best_overall = 0
        for g in range(self.generations):
            battle_win = -1
            for p in range(P):
                dev.unfreeze(t, Path[p])
                if p != battle_win:
                    optim[p] = dev.new_optimizer(lr[p])           # renew the loser's optimizer
                for e in range(self.nepochs):
                    t0 = time.time()
                    dev.train_epoch(t, Path[p], optim[p])
                    ms = 1000 * (time.time() - t0)
                    tr_loss, tr_acc = dev.eval(t, "train", Path[p])
                    va_loss, va_acc = dev.eval(t, "val", Path[p])
                    line = "| Generation {:3d} | Path {:3d} | Epoch {:3d}, time={:7.1f}ms | Train: loss={:.3f}, acc={:5.1f}% | " \
                           "Valid: loss={:.3f}, acc={:5.1f}% |".format(g + 1, p + 1, e + 1, ms, tr_loss, 100 * tr_acc, va_loss,
                                                                        100 * va_acc)
                    if va_acc > best_overall:
                        best_overall = va_acc
                        best_state = dev.snapshot()
                        winner = p
                        line += " B"
                    if va_acc > best_acc[p]:
                        best_acc[p] = va_acc
                        patience[p] = self.lr_patience
                        line += " *"
                    else:
                        patience[p] -= 1
                        if patience[p] == self.lr_patience // 2:  # the LR is divided once; nothing stops a participant
                            lr[p] /= self.lr_factor
                            line += " lr={:.1e}".format(lr[p])
                            dev.set_lr(optim[p], lr[p])
                    self.log(line)
                battle_win = winner
            dev.restore(best_state)
            self.log("| Winning path: {:3d} | Best overall acc: {:.3f} |".format(winner + 1, best_overall))
            probability = 1 / (N * L)
            for p in range(P):
                if p != winner:
                    best_acc[p] = 0
                    lr[p] = lr[winner]
                    patience[p] = self.lr_patience
                    for j in range(L):
                        for k in range(N):
                            Path[p, j, k] = Path[winner, j, k]
                            if np.random.rand() < probability:
                                Path[p, j, k] = (Path[p, j, k] + np.random.randint(-2, 2)) % M
        return Path, winner, best_overall


class Phase1:
    """approaches/pathnet_finetune.py:48-110: one participant over a path that lists every module (the forward uses its
    first N columns).  run() returns (best state or None when no epoch improved, best validation accuracy)."""

    def __init__(self, dev, M, L, nepochs, lr, lr_factor=LR_FACTOR, lr_patience=LR_PATIENCE, log=print):
        self.dev, self.M, self.L, self.nepochs = dev, int(M), int(L), int(nepochs)
        self.lr, self.lr_factor, self.lr_patience = lr, lr_factor, lr_patience
        self.log = log

    def run(self, t):
        dev = self.dev
        if t > 0:
            dev.reinit_modules(t)
        Path = np.random.randint(0, self.M - 1, size=(self.L, self.M))
        for j in range(self.L):
            Path[j, :] = list(range(self.M))
        plan = PatiencePlan(self.lr, self.lr_patience, self.lr_factor, stop_at_or_below_zero=False)
        best_state = None
        dev.unfreeze(t, Path)
        opt = dev.new_optimizer(plan.lr)
        for e in range(self.nepochs):
            t0 = time.time()
            dev.train_epoch(t, Path, opt)
            ms = 1000 * (time.time() - t0)
            tr_loss, tr_acc = dev.eval(t, "train", Path)
            va_loss, va_acc = dev.eval(t, "val", Path)
            line = "| Epoch {:3d}, time={:7.1f}ms | Train: loss={:.3f}, acc={:5.1f}% | Valid: loss={:.3f}, acc={:5.1f}% |".format(
                e + 1, ms, tr_loss, 100 * tr_acc, va_loss, 100 * va_acc)
            verdict = plan.observe(va_acc)
            if verdict == "best":
                best_state = dev.snapshot()
                line += " *"
            elif verdict == "decay":
                line += " lr={:.1e}".format(plan.lr)
                dev.set_lr(opt, plan.lr)
            elif verdict == "stop":
                self.log(line + " [BREAK] Patience=0/{}, with lr={:.1e}".format(self.lr_patience, plan.lr))
                break
            self.log(line)
        return best_state, plan.best


def reinit_modules(net, t):
    """approaches/pathnet.py:83-99: every module that is in no best path of the tasks before t gets the weights of
    net.initial_model back.  Returns the names it re-initialised."""
    done = []
    for offset, (mine, init) in ((0, (net.convs, net.initial_model.convs)), (len(net.convs), (net.fcs, net.initial_model.fcs))):
        for (n, p), (m, q) in zip(mine.named_parameters(), init.named_parameters()):
            assert n == m
            layer, module, _ = n.split(".")
            if int(module) not in net.bestPath[0:t, int(layer) + offset]:
                with torch.no_grad():
                    p.data.copy_(q.data)
                done.append(("convs." if offset == 0 else "fcs.") + n)
    return done


class PathDevice:
    """The device side of both trainers over a PathEngine."""

    def __init__(self, net, loaders, batch_size, in_shape, weight_decay, clipgrad=CLIPGRAD, device="cuda", state_dicts=False):
        self.net, self.loaders, self.wd, self.clipgrad = net, loaders, weight_decay, clipgrad
        self.eng = PN.PathEngine(net, batch_size, in_shape, device)
        self.stats = torch.zeros(2, dtype=torch.float64, device=self.eng.device)          # (sum of batch losses, hits)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=self.eng.device)
        self.state_dicts = state_dicts

    def reinit_modules(self, t):
        reinit_modules(self.net, t)
        self.eng._dirty = True

    def unfreeze(self, t, path):
        self.eng.set_path(path, t)

    def new_optimizer(self, lr):
        return PN.PathSGD(self.eng, lr, MOMENTUM, self.wd)

    def set_lr(self, opt, lr):
        opt.lr = float(lr)

    def train_epoch(self, t, path, opt):
        self.net.train()
        for x, y in self.loaders["train"]:
            self.eng.step(x, y, opt, self.clipgrad)

    def eval(self, t, split, path):
        """(mean CE per sample, accuracy in [0, 1]) as pathnet.py:231-259 weighs them: batch means times batch sizes."""
        self.net.eval()
        self.stats.zero_()
        self.loss_sum.zero_()
        seen = 0
        for x, y in self.loaders[split]:
            loss, _ = self.eng.loss(x, y, stats=self.stats)
            self.loss_sum += loss.double() * x.shape[0]
            seen += x.shape[0]
        return float(self.loss_sum.item()) / seen, float(self.stats[1].item()) / seen

    def snapshot(self):
        # the phase-1 search hands its best state back to the caller as the reference does: a state dict (pathnet_finetune.py:91)
        return deepcopy(self.net.state_dict()) if self.state_dicts else self.eng.snapshot()

    def restore(self, state):
        self.eng.restore(state)


def train_task(net, t, loaders, args, in_shape, device="cuda", log=print):
    """Appr(...).train(t, loaders) of the approach run.py picks; returns what the reference returns."""
    N, M, generations = (int(v) for v in args.parameter)
    assert net.M == M
    if args.finetune_mode:
        dev = PathDevice(net, loaders, args.batch_size, in_shape, args.weight_decay, device=device, state_dicts=True)
        best_model = deepcopy(net)                                 # pathnet_finetune.py:61, handed back when nothing improved
        state, best_acc = Phase1(dev, M, net.L, args.nepochs, args.lr, log=log).run(t)
        best_model = state if state is not None else best_model
        if os.path.exists(args.output):
            torch.save(best_model, os.path.join(args.output, "best_model.pth.tar"))
        return best_model, best_acc
    net.extend_bestPath(N)                                         # pathnet.py:66-81, with the wider array assigned
    dev = PathDevice(net, loaders, args.batch_size, in_shape, args.weight_decay, device=device)
    paths, winner, best_acc = Tournament(dev, N, M, net.L, generations, args.nepochs, args.lr, log=log).run(t)
    net.bestPath[t] = paths[winner]
    torch.save(net, os.path.join(args.output, "best_model.pth.tar"))
    log("-> Saving best model with best paths\n{}".format(net.bestPath[t]))
    return net, best_acc


_DEFAULTS = dict(seed=0, approach="", output="", nepochs=200, save_freq=20, lr=1e10, parameter="")     # run.py:13-22


def main(overwrite_args, device="cuda"):
    """run.py:9-120 for approach == 'pathnet': `overwrite_args` is the dict methods/method.py hands over."""
    tstart = time.time()
    args = SimpleNamespace(**{**_DEFAULTS, **overwrite_args})
    args.task_idx = args.task_count - 1
    if args.approach != "pathnet":
        raise NotImplementedError("Method {} not implemented!".format(args.approach))
    if "VGG" not in args.model_name:
        raise NotImplementedError("PathNet on the HIP path covers the VGG family (vgg_pathnet.py); alexnet_pathnet.py is not "
                                  "built: " + args.model_name)
    dsets = load_task_datasets(args.dataset_path)
    loaders = {x: DeviceLoader(dsets[x], args.batch_size, True, device) for x in ("train", "val")}
    taskcla = list(enumerate(args.nc_per_task))
    inputsize = (3,) + tuple(args.dataset.input_size)
    prev = torch.load(args.prev_model_path, weights_only=False)
    if args.is_scratch_model:
        assert args.task_idx == 0
        net = PN.PathNet(prev, inputsize, taskcla, args.parameter).to(device)
    else:
        net = prev.to(device)
    best_val_model, best_val_acc = train_task(net, args.task_idx, loaders, args, inputsize, device)
    print("[Elapsed time = {:.1f} h]".format((time.time() - tstart) / 3600))
    return best_val_model, best_val_acc
