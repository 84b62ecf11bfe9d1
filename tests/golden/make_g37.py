"""G37: iCaRL — the reference's UNCHANGED methods/rehearsal/model/icarl.py (Net.manage_memory, update_representation,
forward) and its methods/method.py row (dev container only):
    python tests/golden/make_g37.py   ->  tests/golden/G37_icarl.{npz,json}

Harness (G35 pattern): exemplar 'paths' are keys into a tensor bank; the class subsets of manage_memory are datasets over
the task's tensors yielding (image, label, key); RehearsalMemory's image folder becomes (keys, targets) and its loader a real
DataLoader(shuffle=True, num_workers=0) whose fetch order is logged (= the chunk order).  nn.Dropout draws its masks from a
separate torch.Generator and logs them, so that the global CPU generator sees the loaders' draws only.
Sequence: manage_memory(0) on the initial net; WARM_STEPS observe steps at task 2 (not recorded), manage_memory(1); STEPS
recorded observe steps at task 3 (two past tasks, two chunks per task), manage_memory(2).  Recorded: per manage_memory and
class the features in dataset order, the mean weights, the ranking and mem_class_y; per recorded step the host draws
(chunks as (class, exemplar index)), the dropout masks in mixed-batch order, the loss and hits, the CE of the current
batch and every chunk's distillation loss, the gradients of the first
step; parameters before and after the steps; the nearest-mean outputs of every (model, task) on a probe batch.
At every pick the generator ASSERTS that the best untaken cost is at least 1e-4 (relative) below the second best.
The fixture stays independent of the HIP kernels: the reference run is torch on the CPU."""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "harness"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import harness  # noqa: E402

torch = harness.install()
import g37_common as I  # noqa: E402

GAP = 1e-4


def weights(n, bs):
    nb = (n + bs - 1) // bs
    w = np.empty(n, dtype=np.float32)
    for b in range(nb):
        lo, hi = b * bs, min(n, (b + 1) * bs)
        w[lo:hi] = 1.0 / (nb * (hi - lo))
    return w


def check_gaps(feats, mu, ranking, tag):
    """Restates the cost of :422-425 at every pick and asserts the gap; returns the smallest relative gap seen."""
    f = torch.from_numpy(feats)
    taken = np.zeros(len(f), dtype=bool)
    prev = torch.zeros(f.shape[1])
    worst = np.inf
    for k, win in enumerate(ranking):
        cost = (mu.unsqueeze(0) - (f + prev.unsqueeze(0)) / (k + 1)).norm(2, 1).numpy().astype(np.float64)
        cost[taken] = np.inf
        order = np.argsort(cost, kind="stable")
        assert order[0] == win, (tag, k, int(order[0]), int(win))
        if np.isfinite(cost[order[1]]):
            gap = (cost[order[1]] - cost[order[0]]) / cost[order[0]]
            assert gap >= GAP, "pick %d of %s: relative gap %.3g < %.0e — change the seed" % (k, tag, gap, GAP)
            worst = min(worst, gap)
        taken[win] = True
        prev = prev + f[win]
    return worst


def main():
    import methods.rehearsal.model.icarl as IC
    import make_g22 as G22
    import methods.method as RM
    npz, meta = {}, {"constants": I.constants(), "method": G22.describe(RM.parse("ICARL"))}

    class NoWorkers(torch.utils.data.DataLoader):
        def __init__(self, *a, **kw):
            kw["num_workers"] = 0
            kw.pop("pin_memory", None)
            super().__init__(*a, **kw)
    torch.utils.data.DataLoader = NoWorkers

    bank, tasks = {}, []
    for t in range(I.N_TASKS):
        x, y = I.task_data(t)
        tasks.append((torch.from_numpy(x), torch.from_numpy(y)))
        for i in range(len(y)):
            bank["t%d_%d" % (t, i)] = tasks[t][0][i]

    class ClassSubset(torch.utils.data.Dataset):              # ImageFolder_Subset_ClassIncremental + PathRetriever
        def __init__(self, folder, target_idx):
            self.t = folder.task
            self.idx = [i for i in range(len(tasks[self.t][1])) if int(tasks[self.t][1][i]) == target_idx]
            self.label = target_idx

        def __len__(self):
            return len(self.idx)

        def __getitem__(self, i):
            return tasks[self.t][0][self.idx[i]], self.label, "t%d_%d" % (self.t, self.idx[i])
    IC.ImageFolder_Subset_ClassIncremental = ClassSubset
    IC.ImageFolder_Subset_PathRetriever = lambda d: d

    log = {"fetch": [], "folders": [], "masks": []}

    class Folder(torch.utils.data.Dataset):
        def __init__(self, keys, targets):
            self.keys, self.targets = list(keys), targets

        def __len__(self):
            return len(self.keys)

        def __getitem__(self, i):
            log["fetch"].append(i)
            if self.targets is None:
                return bank[self.keys[i]]
            return bank[self.keys[i]], self.targets[i]

    def patch_memory(net):
        md = net.mem_class_x

        def get_imagefolder(exemplarlist, targetlist, transform):
            log["folders"].append(list(exemplarlist))
            return Folder(exemplarlist, targetlist)
        md.get_imagefolder = get_imagefolder
        md.get_dataloader = lambda folder, batch_size=None: torch.utils.data.DataLoader(folder, batch_size=batch_size, shuffle=True)

    mask_gen = torch.Generator()
    mask_gen.manual_seed(I.SEED + 1)

    def dropout_forward(self, inp):
        if not self.training or self.p == 0:
            return inp
        keep = 1.0 - self.p
        mask = torch.bernoulli(torch.full(inp.shape, keep), generator=mask_gen) / keep
        log["masks"].append(mask.numpy().copy())
        return inp * mask
    torch.nn.Dropout.forward = dropout_forward

    torch.manual_seed(I.SEED)
    base = I.make_net()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "base.pth.tar")
    torch.save(base, path)
    args = types.SimpleNamespace(prev_model_path=path, cuda=False, n_memories=I.N_MEMORIES, nc_per_task=I.NC_PER_TASK, lr=I.LR,
                                 weight_decay=I.WD, memory_strength=I.REG, n_outputs=I.N_OUT, n_tasks=I.N_TASKS,
                                 batch_size=I.HERD_BATCH, total_batch_size=I.TOTAL_BATCH,
                                 n_exemplars_to_append_per_batch=I.N_APPEND,
                                 task_imgfolders={"train": types.SimpleNamespace(transform=None, task=0)},
                                 dset_loaders={"train": (tasks[0][0][:2], None, None)})
    net = IC.Net(0, I.N_OUT, I.N_TASKS, args)
    n_drop = sum(1 for m in net.net_classifier.modules() if isinstance(m, torch.nn.Dropout))

    def params(tag):
        for i, p in enumerate(net.parameters()):
            npz["%s_%d" % (tag, i)] = p.detach().numpy().copy()

    def postprocess(t):
        args.task_imgfolders = {"train": types.SimpleNamespace(transform=None, task=t)}
        args.batch_size = I.HERD_BATCH
        net.manage_memory(t, args)
        patch_memory(net)
        o1 = sum(I.NC_PER_TASK[:t])
        rec = {"exemplar_count": net.exemplar_count, "classes": []}
        for c in range(I.NC_PER_TASK[t]):
            sub = ClassSubset(args.task_imgfolders["train"], c)
            xs = torch.stack([sub[i][0] for i in range(len(sub))])
            with torch.no_grad():
                feats = net.get_feature(xs).numpy().copy()
                mu = torch.stack([net.get_feature(xs[s:s + I.HERD_BATCH]).mean(0) for s in range(0, len(xs), I.HERD_BATCH)]).mean(0)
            keys = net.mem_class_x[o1 + c]
            where = {"t%d_%d" % (t, j): i for i, j in enumerate(sub.idx)}
            ranking = [where[k] for k in keys]
            gap = check_gaps(feats, mu, ranking, "task %d class %d" % (t, c))
            npz["m%d_c%d_feats" % (t, c)] = feats
            npz["m%d_c%d_w" % (t, c)] = weights(len(sub), I.HERD_BATCH)
            npz["m%d_c%d_y" % (t, c)] = net.mem_class_y[o1 + c].numpy().copy()
            rec["classes"].append({"rows": sub.idx, "ranking": ranking, "min_gap": float(gap)})
        rec["lengths"] = {str(k): len(v) for k, v in net.mem_class_x.exemplars.items()}
        meta["manage"].append(rec)
        # nearest-mean outputs of this model for every task
        args.batch_size = I.EVAL_BATCH
        probe = torch.from_numpy(I.probe_batch())
        net.train(False)
        for task in range(I.N_TASKS):
            with torch.no_grad():
                npz["nme_m%d_t%d" % (t, task)] = net.forward(probe, task, args).numpy().copy()
        net.train(True)

    def logged(module, key, factor):
        inner = module.forward

        def forward(*a, **kw):
            out = inner(*a, **kw)
            log[key].append(float(out.item()) * factor)
            return out
        module.forward = forward
    logged(net.ce, "ce", 1.0)
    logged(net.kl, "kl", 4.0)                                  # the chunk loss is kl * T ** 2 (:581), T = 2

    def observe(t, x, y):
        log["fetch"], log["folders"], log["masks"], log["ce"], log["kl"] = [], [], [], [], []
        patch_memory(net)
        args.task_imgfolders = {"train": types.SimpleNamespace(transform=None, task=t)}
        loss, hits, _ = net.observe(torch.from_numpy(x), t, torch.from_numpy(y), None, args)
        where = {key: (c, e) for c, keys in net.mem_class_x.exemplars.items() for e, key in enumerate(keys)}
        plan, fi = [], 0
        for folder in log["folders"]:
            order = log["fetch"][fi:fi + len(folder)]
            fi += len(folder)
            ordered = [list(where[folder[i]]) for i in order]
            task = max(k for k in range(I.N_TASKS) if sum(I.NC_PER_TASK[:k]) <= ordered[0][0])
            plan.append({"task": task, "rows": [list(where[k]) for k in folder],
                         "chunks": [ordered[j:j + I.TOTAL_BATCH] for j in range(0, len(ordered), I.TOTAL_BATCH)]})
        per = [np.concatenate(log["masks"][d::n_drop]) for d in range(n_drop)]      # mixed-batch order: current | chunks
        return float(loss.item()), int(hits), plan, per

    meta["manage"] = []
    params("p_init")
    postprocess(0)
    net.init_setup(args)
    I.seed_draws(1)
    for x, y in I.step_batches(1, I.WARM_STEPS):
        observe(1, x, y)
    params("p_task2")
    postprocess(1)
    net.init_setup(args)
    I.seed_draws(2)
    meta["steps"] = []
    for k, (x, y) in enumerate(I.step_batches(2, I.STEPS)):
        loss, hits, plan, masks = observe(2, x, y)
        # (float64 of fp32 values: the CE of the current batch and every chunk's T^2 KL in loader order, tasks ascending)
        meta["steps"].append({"loss": loss, "hits": hits, "plan": plan, "ce": log["ce"][0], "chunk_losses": list(log["kl"])})
        for d, m in enumerate(masks):
            npz["s%d_mask%d" % (k, d)] = m
        if k == 0:
            for i, p in enumerate(net.parameters()):
                npz["s0_grad_%d" % i] = p.grad.detach().numpy().copy()
    params("p_task3")
    postprocess(2)
    np.savez_compressed(os.path.join(HERE, "G37_icarl.npz"), **npz)
    with open(os.path.join(HERE, "G37_icarl.json"), "w") as f:
        json.dump(meta, f, indent=0)
    for rec in meta["manage"]:
        print(rec["exemplar_count"], rec["lengths"], [round(c["min_gap"], 5) for c in rec["classes"]])
    for s in meta["steps"]:
        print(round(s["loss"], 5), s["hits"], [(p["task"], [len(c) for c in p["chunks"]]) for p in s["plan"]])


if __name__ == "__main__":
    main()
