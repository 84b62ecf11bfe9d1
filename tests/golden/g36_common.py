"""Shared by the G36 generator (reference run, dev container) and the tests of the Joint baseline: the cases, the stand-in
method / dataset objects, and the routines that run ONE implementation (passed in) over them."""
import os
import shutil
import tempfile
from collections import OrderedDict
from types import SimpleNamespace

import torch

MODEL = "small_VGG9_cl_128_128"
# tiny3 (the sequence of G10 / G17 / G33): 3 tasks x 4 classes, 160 / 40 / 40 images of 3x32x32
TINY3 = dict(task_count=3, classes_per_task=4, sizes=(160, 40, 40), hw=32, noise=0.4, name="tiny3")
# The grid of the end-to-end run.  Chosen so that the reference reproduces itself: two CPU runs with different reduction
# orders (one thread / default threads) agree per LR to within one validation image and on the winner (make_g36.py checks
# this before it records anything and stores both runs).
LR_GRID = "1e-2,3e-3"
NUM_EPOCHS = 24
BATCH = 40
COMMON = [MODEL, "--lr_grid", LR_GRID, "--num_epochs", str(NUM_EPOCHS), "--batch_size", str(BATCH), "--saving_freq", "100"]

HOOKS = ["train", "grid_train", "grid_prestep", "grid_poststep", "grid_datafetch", "compose_dataset", "prestep", "poststep",
         "train_args_overwrite", "train_init", "init_next_task", "get_output", "inference_eval", "eval_model_preprocessing"]
ROW_FIELDS = ("name", "eval_name", "category", "extra_hyperparams_count", "hyperparams", "static_hyperparams")


def plain(v):
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, dict):
        return [[str(k), plain(x)] for k, x in v.items()]
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return "<%s>" % type(v).__name__


# ---------------------------------------------------------------------------------------------- 1. the method row
def describe(m):
    """What G22 records per method."""
    cat = m.category
    return {"class": type(m).__name__, "name": m.name, "eval_name": m.eval_name,
            "category": getattr(cat, "name", str(cat)), "extra_hyperparams_count": m.extra_hyperparams_count,
            "hyperparams": plain(m.hyperparams), "static_hyperparams": plain(getattr(m, "static_hyperparams", None)),
            "flags": {k: getattr(m, k) for k in sorted(dir(m))
                      if not k.startswith("_") and k not in ROW_FIELDS and k not in vars(m)
                      and isinstance(getattr(m, k), (bool, int, float, str))},
            "hooks": [h for h in HOOKS if callable(getattr(m, h, None))]}


def get_output_error(m):
    try:
        m.get_output(None, None)
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None


class PathDataset:
    """Task sequence of three files; `joint` is the pre-merged file of all tasks, or None."""
    task_count = 3

    def __init__(self, joint=None):
        self.joint, self.calls = joint, []

    def get_taskname(self, i):
        return str(i)

    def get_task_dataset_path(self, task_name=None, rnd_transform=False):
        self.calls.append([task_name, rnd_transform])
        return self.joint if task_name is None else "task_%s.pth" % task_name


def hooks(m):
    """train_args_overwrite and grid_datafetch of a method object, as data."""
    args = SimpleNamespace(starting_task_count=2, max_task_count=3, task_name="1")
    m.train_args_overwrite(args)
    out = {"args_after_overwrite": [args.starting_task_count, args.max_task_count], "datafetch": []}
    for joint in (None, "all_tasks.pth"):
        ds = PathDataset(joint)
        out["datafetch"].append({"joint_file": joint, "returns": m.grid_datafetch(args, ds), "asked": ds.calls})
    return out


def phase1_call(m, fine_tune_holder, attr="fine_tune_SGD"):
    """grid_train of a method object with compose_dataset and the SGD trainer replaced by recorders: the dataset list handed
    to compose_dataset and the keyword arguments of the trainer call (what G28 records for the other methods)."""
    seen = {}

    def compose(dataset_path, batch_size, *a, **k):
        seen["compose"] = [list(dataset_path), batch_size]
        return "LOADERS", "SIZES", "CLASSES"

    def trainer(*a, **k):
        seen["positional"] = list(a)
        seen["keywords"] = {key: k[key] for key in sorted(k) if key not in ("device", "batch_size")}
        return "MODEL", 0.5

    args = SimpleNamespace(batch_size=40, num_epochs=8, weight_decay=0.0, saving_freq=100, device="cpu")
    manager = SimpleNamespace(current_task_dataset_path=["a.pth", "b.pth", "c.pth"], previous_task_model_path="base.pth.tar",
                              gridsearch_exp_dir="node_dir", method=m)
    old = getattr(fine_tune_holder, attr)
    setattr(fine_tune_holder, attr, trainer)
    try:
        restore = _swap_compose(m, compose)
        try:
            seen["returns"] = list(m.grid_train(args, manager, 0.003))
        finally:
            restore()
    finally:
        setattr(fine_tune_holder, attr, old)
    return seen


def _swap_compose(m, compose):
    """Both implementations reach compose_dataset through a class attribute: the reference's Joint.grid_train calls
    Finetune.compose_dataset, the build's calls the method's own hook."""
    owners = [c for c in type(m).__mro__ if "compose_dataset" in vars(c)]
    import sys
    mod = sys.modules[type(m).__module__]
    ft = getattr(mod, "Finetune", None)
    if ft is not None and ft not in owners and "compose_dataset" in vars(ft):
        owners.append(ft)
    saved = [(c, vars(c)["compose_dataset"]) for c in owners]
    for c in owners:
        setattr(c, "compose_dataset", staticmethod(compose))

    def restore():
        for c, v in saved:
            setattr(c, "compose_dataset", v)
    return restore


# ---------------------------------------------------------------------------------------------- 2. the evaluation loop
class Split(torch.utils.data.Dataset):
    """One split of a stand-in task file: a class list and one 1-pixel image."""

    def __init__(self, classes):
        self.classes = list(classes)

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return torch.zeros(1), 0


TASK_CLASSES = [["t0c0", "t0c1", "t0c2"], ["t1c0", "t1c1"], ["t2c0", "t2c1", "t2c2", "t2c3"]]       # uneven on purpose
ALL_CLASSES = [c for t in TASK_CLASSES for c in t]
SHUFFLED = [ALL_CLASSES[i] for i in (5, 0, 7, 3, 8, 1, 6, 2, 4)]        # the joint file's own (unsorted) class order
ACC = [91.25, 62.5, 77.0]
SINGLE_CASES = [
    dict(tag="by_count", joint=None, start=1, stop=3, fail=None, debug=False),
    dict(tag="by_name", joint=SHUFFLED, start=1, stop=3, fail=None, debug=False),
    dict(tag="class_count_mismatch", joint=SHUFFLED + ["stranger"], start=1, stop=3, fail=None, debug=False),
    dict(tag="window", joint=None, start=2, stop=3, fail=None, debug=False),
    dict(tag="fails", joint=SHUFFLED, start=1, stop=3, fail=1, debug=False),
    dict(tag="debug", joint=None, start=1, stop=3, fail=None, debug=True),
]


class SingleModelMethod:
    name = eval_name = "standin_joint"

    def __init__(self, task_paths, joint_path, fail):
        self.task_paths, self.joint_path, self.fail, self.calls, self.composed = task_paths, joint_path, fail, [], []

    def grid_datafetch(self, args, dataset):
        return self.joint_path if self.joint_path is not None else list(self.task_paths)

    def compose_dataset(self, dataset_path, batch_size, *a, **k):
        self.composed.append([os.path.basename(p) for p in dataset_path])
        sizes = [len(c) for c in TASK_CLASSES]
        cum = [sum(sizes[:i + 1]) for i in range(len(sizes))]
        loader = SimpleNamespace(dataset=SimpleNamespace(cumulative_classes_len=cum))
        return {"train": loader, "val": loader}, None, {"train": [list(c) for c in TASK_CLASSES], "val": [list(c) for c in TASK_CLASSES]}

    def inference_eval(self, args, manager):
        self.calls.append([args.dataset_index, os.path.basename(args.dataset_path), [list(t) for t in args.tasks_idxes]])
        if self.fail is not None and args.dataset_index == self.fail:
            raise RuntimeError("evaluation of this task fails")
        return ACC[args.dataset_index]


def single_evals(eval_single_model_all_tasks, perf_filename):
    """`perf_filename()` -> the joint result file's name for an eval_name."""
    out = []
    for c in SINGLE_CASES:
        root = tempfile.mkdtemp()
        try:
            data, res = os.path.join(root, "data"), os.path.join(root, "out")
            os.makedirs(data)
            os.makedirs(res)
            task_paths = []
            for i, classes in enumerate(TASK_CLASSES):
                task_paths.append(os.path.join(data, "task_%d.pth" % (i + 1)))
                torch.save({"train": Split(classes), "val": Split(classes)}, task_paths[-1])
            joint_path = None
            if c["joint"] is not None:
                joint_path = os.path.join(data, "joint.pth")
                torch.save({"train": Split(c["joint"]), "val": Split(c["joint"])}, joint_path)
            meth = SingleModelMethod(task_paths, joint_path, c["fail"])
            mgr = SimpleNamespace(method=meth, dataset=SimpleNamespace(task_count=len(task_paths)))
            args = SimpleNamespace(test_starting_task_count=c["start"], test_max_task_count=c["stop"], out_path=res,
                                   debug=c["debug"], batch_size=40, device="cpu")
            raised = None
            try:
                eval_single_model_all_tasks(args, mgr, list(task_paths))
            except (Exception, AssertionError) as e:
                raised = type(e).__name__
            files = OrderedDict()
            for f in sorted(os.listdir(res)):
                files[f] = plain(torch.load(os.path.join(res, f), weights_only=False))
            out.append({"tag": c["tag"], "raises": raised, "calls": meth.calls, "composed": meth.composed, "files": files,
                        "expected_file": perf_filename(meth.eval_name),
                        "task_counter": getattr(args, "task_counter", None), "task_name": getattr(args, "task_name", None)})
        finally:
            shutil.rmtree(root)
    return out
