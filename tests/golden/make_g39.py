"""G39: host logic of the PathNet trainers as DATA, from the reference's UNCHANGED approaches/pathnet.py and
approaches/pathnet_finetune.py (dev container only, CPU).

Appr.train of both approaches runs for t = 0 and t = 1 over the reference's own vgg_pathnet.Net (tiny), with train_epoch
and eval replaced by scripted stand-ins: an epoch only advances a counter buffer of the model (so every saved / restored
state can be told apart), validation accuracies come from a recorded table.  Under a fixed np.random.seed the fixture
records the sequence of events — reinit, unfreeze (path, trainable set), optimizer creations with their LR, per epoch the
optimizer in use (ordinal of its creation) and its LR, saves and restores of the best state (counter value), LR changes —
the final bestPath, the return value, the next draw of the generator, and the method-table row of `pathnet` as G22 has it
for the other methods.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "harness"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import harness  # noqa: E402

torch = harness.install()
if not hasattr(np, "int"):
    np.int = int                                   # vgg_pathnet.py:94 predates NumPy 1.24
import g38_common as G  # noqa: E402
import g39_common as S  # noqa: E402
import make_g22 as G22  # noqa: E402
import make_g38 as G38  # noqa: E402


def accuracies(seed, n):
    """Validation accuracies in steps of 0.05: ties and plateaus are frequent."""
    return [float(v) for v in np.round(np.random.RandomState(seed).uniform(0.2, 0.9, size=n) * 20) / 20]


def run(kind, t, net, acc_table):
    import methods.HAT.HAT_utils as HU
    import methods.HAT.approaches.pathnet as AP
    import methods.HAT.approaches.pathnet_finetune as APF
    events = []
    args = types.SimpleNamespace(parameter=[S.N, S.M, S.GENERATIONS], weight_decay=G.WD)
    mod = AP if kind == "joint" else APF
    appr = mod.Appr(net, os.path.join(tempfile.gettempdir(), "g39_no_such_dir"), nepochs=S.NEPOCHS if kind == "joint" else S.PHASE1_EPOCHS,
                    sbatch=40, lr=S.LR, lr_factor=S.LR_FACTOR, lr_patience=S.LR_PATIENCE, args=args)
    if not hasattr(net, "ticks"):
        net.register_buffer("ticks", torch.zeros(1))
    made, accs = [], iter(acc_table)
    own = lambda: [(n, p) for n, p in net.named_parameters() if not n.startswith("initial_model.")]   # noqa: E731

    get_opt, unfreeze, reinit = appr._get_optimizer, net.unfreeze_path, appr.reinit_modules
    get_state, set_state, set_lr, save = HU.get_model_state, HU.set_model_state_, HU.set_lr_, torch.save

    def new_optimizer(lr=None):
        o = get_opt(lr)
        made.append(o)
        events.append(["optim", o.param_groups[0]["lr"]])
        return o

    def unfreeze_path(tt, Path):
        unfreeze(tt, Path)
        names = sorted(n for n, p in own() if p.requires_grad and not n.startswith("classifier"))
        events.append(["unfreeze", np.asarray(Path).tolist(), names])

    def reinit_modules(tt):
        with torch.no_grad():
            for n, p in own():
                p.add_(1.0)                       # away from initial_model, so that what reinit copies back shows
        reinit(tt)
        init = dict(net.initial_model.named_parameters())
        events.append(["reinit", tt, sorted(n for n, p in own() if torch.equal(p, init[n]))])

    def train_epoch(tt, loader, Path, use_gpu=True):
        assert loader == ("train",)
        net.ticks += 1
        events.append(["train", [i for i, o in enumerate(made) if o is appr.optimizer][0], appr.optimizer.param_groups[0]["lr"]])

    def evaluate(tt, loader, Path=None, use_gpu=True):
        events.append(["eval", loader[0]])
        return (1.0, next(accs)) if loader == ("val",) else (1.0, 0.0)

    def get_model_state(model):
        events.append(["save", float(model.ticks)])
        return get_state(model)

    def set_model_state_(model, state):
        events.append(["restore", float(state["ticks"])])
        return set_state(model, state)

    def set_lr_(opt, lr):
        events.append(["set_lr", [i for i, o in enumerate(made) if o is opt][0], lr])
        return set_lr(opt, lr)

    def torch_save(obj, path):
        events.append(["torch.save", type(obj).__name__, os.path.basename(path)])

    appr._get_optimizer, net.unfreeze_path, appr.reinit_modules = new_optimizer, unfreeze_path, reinit_modules
    appr.train_epoch, appr.eval = train_epoch, evaluate
    HU.get_model_state, HU.set_model_state_, HU.set_lr_, torch.save = get_model_state, set_model_state_, set_lr_, torch_save
    np.random.seed(S.SEEDS["%s_t%d" % (kind, t)])
    try:
        best_model, best_acc = appr.train(t, {"train": ("train",), "val": ("val",)})
    finally:
        HU.get_model_state, HU.set_model_state_, HU.set_lr_, torch.save = get_state, set_state, set_lr, save
        del net.unfreeze_path
    return {"events": events, "best_acc": float(best_acc), "returns": type(best_model).__name__,
            "bestPath": np.asarray(net.bestPath).tolist(), "rng_after": float(np.random.rand()),
            "ticks": float(net.ticks), "val_acc": acc_table}


def main():
    import methods.method as RM
    out = {"constants": {k: getattr(S, k) for k in ("N", "M", "L", "GENERATIONS", "NEPOCHS", "LR", "LR_FACTOR", "LR_PATIENCE",
                                                    "PHASE1_EPOCHS", "SEEDS")}}
    m = RM.Pathnet()                               # (the reference's parse() has no branch for it; the class is there)
    row = G22.describe(m)
    row["decay_operator"] = [[a, m.decay_operator(a, 1)] for a in (2, 3, 3.0)]
    out["method"] = row
    net, _, _ = G38.build("a", torch.float32)
    n_joint = S.GENERATIONS * 2 * (S.NEPOCHS // S.GENERATIONS)
    out["joint_t0"] = run("joint", 0, net, accuracies(1, n_joint))
    out["joint_t1"] = run("joint", 1, net, accuracies(2, n_joint))
    net, _, _ = G38.build("a", torch.float32)
    out["phase1_t0"] = run("phase1", 0, net, accuracies(3, S.PHASE1_EPOCHS))
    net.bestPath[0] = np.array(out["joint_t0"]["bestPath"][0])
    out["phase1_t1"] = run("phase1", 1, net, accuracies(4, S.PHASE1_EPOCHS))
    dst = os.path.join(HERE, "G39_pathnet_trainer.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
    for k in ("joint_t0", "joint_t1", "phase1_t0", "phase1_t1"):
        r = out[k]
        print(k, len(r["events"]), "events", "best", r["best_acc"], r["returns"], "lr events",
              [e for e in r["events"] if e[0] == "set_lr"], "ticks", r["ticks"])
    print(os.path.getsize(dst) // 1024, "KiB")


if __name__ == "__main__":
    main()
