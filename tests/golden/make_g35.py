"""G35: the rehearsal baselines — the reference's UNCHANGED methods/rehearsal/model/baseline_rehearsal_{partial,full}_mem.py
(Net.observe_FT), main_rehearsal.main and methods/method.py rows (dev container only):
    python tests/golden/make_g35.py   ->  tests/golden/G35_rehearsal_baselines.{npz,json}

Runs (G15 harness pattern): exemplar 'paths' are keys into a tensor bank; RehearsalMemory's image folder becomes
(keys, labels) and its loader a real DataLoader(shuffle=True, num_workers=0) over the banked tensors, whose fetch order is
logged (= the chunk order).  Dropout masks are drawn from a separate torch.Generator so that the global CPU generator
sees what a CUDA run's would (the head init and the exemplar loaders' draws only).  Recorded per step: exemplar slots and
chunk orders per past task, mask rows, loss, hits, memory labels, mem_cnt, n_memories; parameters at the end of each task.
  a  partial memory, BN-free VGG-structured net with dropout, 3 tasks; n_append > chunk size at task 1 (count > t)
  b  full memory, 3 tasks (truncation at each switch)
  c  partial memory, the same net with BatchNorm
main_rehearsal.main with train_model replaced by a recorder: (loader batch size, chunk size, n_append) for both methods
at tasks 1-3.  method.py: G22-style rows and G28-style trainer arguments of both classes; the harness supplies
manager.datasets (data.dataset) and args.mem_per_task, which the reference lacks, and makes the top-level `model`
package importable (main_rehearsal.py:214).
The reference Net torch.load()s its base net; that module is the build's clsurvey_amd.models.VGGSlim (g35_common.make_net),
so the torch forward of these runs is the build's module definition, which G34 pins to the reference's model factory.
The fixture stays independent of the HIP kernels: the reference run is torch on the CPU."""
import contextlib
import json
import os
import random
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
import g35_common as I  # noqa: E402


def run(tag, spec):
    import methods.rehearsal.model.baseline_rehearsal_partial_mem as PM
    out = {}
    torch.manual_seed(spec["seed"])
    base = I.make_net(spec["bn"])
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "base.pth.tar")
    torch.save(base, path)
    args = types.SimpleNamespace(prev_model_path=path, cuda=False, n_memories=spec["n_memories"], nc_per_task=I.NC_PER_TASK,
                                 lr=I.LR, weight_decay=I.WD, full_mem_mode=spec["full"], batch_size=1,
                                 n_exemplars_to_append_per_batch=0,
                                 task_imgfolders={"train": types.SimpleNamespace(transform=None)})
    net = PM.Net(0, I.N_OUT, I.N_TASKS, args)
    net.memory_labels.zero_()              # uninitialised LongTensor in the reference; only filled slots are ever read
    for i, p in enumerate(net.parameters()):
        out["%s_p0_%d" % (tag, i)] = p.detach().numpy().copy()
    bank = {}
    mask_gen = torch.Generator()
    mask_gen.manual_seed(spec["seed"] + 1)
    orig_bernoulli = torch.bernoulli
    torch.manual_seed(spec["seed"] + 2)
    random.seed(spec["seed"] + 3)
    log = {}

    class Folder(torch.utils.data.Dataset):
        def __init__(self, keys, labels):
            self.keys, self.labels = list(keys), labels.clone()

        def __len__(self):
            return len(self.keys)

        def __getitem__(self, i):
            log["fetch"].append(i)
            return bank[self.keys[i]], self.labels[i]

    def patch_memory():
        md = net.memory_data

        def get_imagefolder(exemplarlist, targetlist, transform):
            log["folders"].append(list(exemplarlist))
            return Folder(exemplarlist, targetlist)
        md.get_imagefolder = get_imagefolder
        md.get_dataloader = lambda folder, batch_size=None: torch.utils.data.DataLoader(folder, batch_size=batch_size,
                                                                                        shuffle=True, num_workers=0)
    data = I.batches(spec["seed"] + 4)
    steps = []
    k = 0
    for t in range(I.N_TASKS):
        net.init_setup(args)                        # main() at every task
        net.train(True)
        args.n_exemplars_to_append_per_batch, args.batch_size = spec["append"][t]
        for s in range(I.STEPS):
            x, y = data[k]
            x, y = torch.from_numpy(x), torch.from_numpy(y)
            keys = [(k, i) for i in range(len(y))]
            for kk, xi in zip(keys, x):
                bank[kk] = xi
            log["fetch"], log["folders"] = [], []
            if net.memory_data is not None:
                patch_memory()
            torch.bernoulli = lambda inp, *a, **kw: orig_bernoulli(inp, generator=mask_gen)
            try:
                loss, hits = net.observe_FT(x, t, y, keys, args)
            finally:
                torch.bernoulli = orig_bernoulli
            patch_memory()
            slot_of = {}
            for task in range(I.N_TASKS):
                for slot, key in enumerate(net.memory_data.exemplars[task][:net.n_memories]):
                    if key is not None:
                        slot_of[(task, key)] = slot
            rec = {"t": t, "loss": float(loss.item()), "hits": int(hits), "mem_cnt": net.mem_cnt, "n_memories": net.n_memories,
                   "plan": []}
            fetch = list(log["fetch"])
            fi = 0
            for folder in log["folders"]:
                task = folder[0][0] // I.STEPS                   # bank key = (global step, row)
                slots = [slot_of[(task, key)] for key in folder]
                order = fetch[fi:fi + len(folder)]
                fi += len(folder)
                ordered = [slots[i] for i in order]
                cbs = args.batch_size
                rec["plan"].append({"task": task, "slots": slots,
                                    "chunks": [ordered[j:j + cbs] for j in range(0, len(ordered), cbs)]})
            steps.append(rec)
            for idx in sorted(net.dropout_masks):
                out["%s_s%d_mask%d" % (tag, k, idx)] = net.dropout_masks[idx].numpy().copy()
            out["%s_s%d_mem_labels" % (tag, k)] = net.memory_labels.numpy().copy()
            k += 1
        for i, p in enumerate(net.parameters()):
            out["%s_p_task%d_%d" % (tag, t, i)] = p.detach().numpy().copy()
    return out, steps


def triples():
    """main_rehearsal.main -> (loader batch size, chunk size, n_append) for both methods, tasks 1-3."""
    import methods.rehearsal.main_rehearsal as MR
    import methods.rehearsal.train_rehearsal as TR
    import methods.rehearsal.model as model_pkg
    sys.modules.setdefault("model", model_pkg)                 # main_rehearsal.py:214 imports 'model.<method>'
    tmp = tempfile.mkdtemp()
    dpath = os.path.join(tmp, "task.pth")
    dsets = {"train": torch.utils.data.TensorDataset(torch.zeros(I.TRIPLE_TRAIN, 1)),
             "val": torch.utils.data.TensorDataset(torch.zeros(7, 1))}
    torch.save(dsets, dpath)
    torch.manual_seed(0)
    mpath = os.path.join(tmp, "base.pth")
    torch.save(I.make_net(False), mpath)
    seen = {}
    saved = (TR.train_model, MR.ImageFolder_Subset_PathRetriever, sys.argv)

    def recorder(model, args, dset_sizes, resume=""):
        seen["r"] = (args.dset_loaders["train"].batch_size, args.batch_size, args.n_exemplars_to_append_per_batch)
        return None, 0.0
    TR.train_model = recorder
    MR.ImageFolder_Subset_PathRetriever = lambda d: d          # harness: the loaders' dataset wrapper (paths) is not needed
    sys.argv = ["main_rehearsal.py", dpath]
    out = {}
    try:
        for method in ("baseline_rehearsal_partial_mem", "baseline_rehearsal_full_mem"):
            prev = mpath
            for task in (1, 2, 3):
                seen.clear()
                kw = dict(weight_decay=0.0, task_name=str(task), task_count=task, prev_model_path=prev, save_path=tmp,
                          n_outputs=I.TRIPLE_NC * I.TRIPLE_TASKS, method=method, n_memories=I.TRIPLE_MEM, n_epochs=1,
                          cuda=True, dataset_path=dpath, n_tasks=I.TRIPLE_TASKS, batch_size=I.TRIPLE_BATCH, lr=0.01,
                          finetune=True, is_scratch_model=task == 1)
                MR.main(kw, [I.TRIPLE_NC] * I.TRIPLE_TASKS)
                out["%s/task%d" % (method, task)] = list(seen["r"])
                if task == 1:                                  # later tasks load a wrapper
                    import model.baseline_rehearsal_partial_mem as PMm
                    a = types.SimpleNamespace(full_mem_mode=False, prev_model_path=mpath, cuda=False, lr=0.01, weight_decay=0.0,
                                              n_memories=I.TRIPLE_MEM, nc_per_task=[I.TRIPLE_NC] * I.TRIPLE_TASKS)
                    prev = os.path.join(tmp, "wrapper.pth")
                    torch.save(PMm.Net(0, I.TRIPLE_NC * I.TRIPLE_TASKS, I.TRIPLE_TASKS, a), prev)
    finally:
        TR.train_model, MR.ImageFolder_Subset_PathRetriever, sys.argv = saved
    return out


def method_rows():
    import framework.main as FM
    import methods.method as RM
    import data.dataset as DD
    import g28_common as G
    import make_g22 as G22
    rows = {name: G22.describe(RM.parse(name)) for name in I.NAMES}
    for name in I.NAMES:
        rows[name]["arg_string"] = RM.parse(name).arg_string
    MAINS = [(RM.trainRehearsal, "rehearsal.main", (None, 0.5))]

    @contextlib.contextmanager
    def patches(log):
        saved = [(mod, mod.main) for mod, _, _ in MAINS]
        for mod, label, res in MAINS:
            mod.main = G.Recorder(log, label, None, res)
        try:
            yield
        finally:
            for mod, orig in saved:
                mod.main = orig
    FM.Manager.datasets = DD                                   # harness: method.py:1143 reads manager.datasets
    saved = (G.METHODS, G.make_args)
    G.METHODS = list(I.NAMES)
    G.make_args = lambda task, _m=G.make_args: I.with_mem(_m(task))
    try:
        hooks = G.run(RM.parse, FM.Manager, patches, set())
    finally:
        G.METHODS, G.make_args = saved
        del FM.Manager.datasets
    return {"methods": rows, "hooks": hooks}


def main():
    npz, meta = {}, {"runs": {}, "constants": I.constants()}
    for tag, spec in I.RUNS.items():
        arrs, steps = run(tag, spec)
        npz.update(arrs)
        meta["runs"][tag] = steps
    meta["triples"] = triples()
    meta.update(method_rows())
    np.savez_compressed(os.path.join(HERE, "G35_rehearsal_baselines.npz"), **npz)
    with open(os.path.join(HERE, "G35_rehearsal_baselines.json"), "w") as f:
        json.dump(meta, f, indent=0)
    for tag, steps in meta["runs"].items():
        print(tag, [(s["t"], round(s["loss"], 4), s["hits"], [len(p["chunks"]) for p in s["plan"]]) for s in steps])
    print(meta["triples"])


if __name__ == "__main__":
    main()
