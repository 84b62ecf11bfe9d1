"""Test-time evaluation — mirror of src/framework/inference.py:8-87 and utils.get_prev_heads
(utilities/utils.py:235-262): swap the task head in, forward the test split, top-1 accuracy x100."""
import copy
from types import SimpleNamespace

import torch

from ..data import DeviceLoader, load_task_datasets
from ..methods import train_common as tc


def get_prev_heads(prev_head_model_paths, head_layer_idx, device="cuda"):
    if not isinstance(prev_head_model_paths, list):
        prev_head_model_paths = [prev_head_model_paths]
    heads = []
    for path in prev_head_model_paths:
        m = tc.load_model(path)
        if isinstance(m, dict):
            m = m["model"]
        head = m.classifier._modules[head_layer_idx]
        assert isinstance(head, torch.nn.Linear), type(head)
        heads.append(copy.deepcopy(head.to(device)))
    return heads


def test_model(method, model, dataset_path, target_task_head_idx, target_head=None, batch_size=200, subset="test",
               per_class_stats=False, final_layer_idx=None, task_idx=None, device="cuda"):
    """Top-1 accuracy (percent) of `model` on one split of a task file, through `method.get_output(images, holder)` —
    the contract of framework/inference.py:8-87: `holder` carries the model, the separately saved heads (`target_head`,
    in which case the head index addresses that list) or the wrapper's own head index, and the classifier's last slot.
    Images stay on the device; hits are counted there and read once."""
    heads = None if target_head is None else (target_head if isinstance(target_head, list) else [target_head])
    if heads is not None:                                    # inference.py:15-18
        assert target_task_head_idx == 0, "Only EBLL, LWF have heads in model itself, here head idx indicates target_headlist idx"
    if hasattr(model, "classifier"):
        final_layer_idx = str(len(model.classifier._modules) - 1)
    model.eval()
    model = model.to(device)
    dsets = load_task_datasets(dataset_path)
    split = subset if "test" in dsets else "val"            # a task file without a test split is scored on val (inference.py:27-33)
    holder = SimpleNamespace(task_imgfolders=dsets, batch_size=batch_size, model=model, heads=heads,
                             current_head_idx=target_task_head_idx, final_layer_idx=final_layer_idx, task_idx=task_idx)
    hits = torch.zeros((), dtype=torch.int64, device=device)
    seen = 0
    for images, labels in DeviceLoader(dsets[split], batch_size, True, device):
        hits += (method.get_output(images, holder).argmax(1) == labels).sum()
        seen += labels.shape[0]
    accuracy = 100.0 * float(hits.item()) / seen
    print("Overall Accuracy: " + str(accuracy))
    return accuracy


def test_task_joint_model(model_path, dataset_path, task_idx, task_lengths, batch_size=200, subset="test", tasks_idxes=None,
                          device="cuda", per_class_stats=False):
    """Accuracy (percent) of ONE task in a model trained jointly on all tasks — framework/inference.py:90-164: shared output
    layer, the outputs of the other tasks are left out: arg-max inside `tasks_idxes[task_idx]` (or, without it, the
    contiguous slice the class counts `task_lengths` give) against the task-local label.  Per batch one plan forward and
    one clhip_slice_argmax_count launch; the per-class counters stay on the device and are read once per task.
    per_class_stats=True returns (accuracy, correct[K], total[K]).  The counters have one entry per output index of the
    slice, K = len(tasks_idxes[task_idx]), and a label outside [0, K) raises IndexError.  The reference sizes its counters by
    the task's own class list instead; the two differ only when the by-name mapping drops classes the joint file does not
    have: there the reference counts such a label as a miss, this stops."""
    from .. import ops
    from ..net import NetEngine
    print("==> TESTING TASK {}".format(task_idx + 1))
    model = tc.load_model(model_path)
    model.eval()
    model = model.to(device)
    dsets = load_task_datasets(dataset_path, device)
    split = subset if "test" in dsets else "val"            # a task file without a test split is scored on val (:113-120)
    if tasks_idxes is None:
        cols = [c + sum(task_lengths[0:task_idx]) for c in range(task_lengths[task_idx])]
    else:
        cols = tasks_idxes[task_idx]
        assert isinstance(cols, list)
    loader = DeviceLoader(dsets[split], batch_size, True, device)
    engine = NetEngine(model, batch_size, tuple(loader.x.shape[1:]), device)
    if not cols or min(cols) < 0 or max(cols) >= engine.n_classes:
        raise IndexError("task %d: output indices %s outside the model's %d outputs" % (task_idx + 1, cols, engine.n_classes))
    K = len(cols)
    cols_dev = torch.tensor(cols, dtype=torch.int32).to(device)
    counters = torch.zeros(2 * K + 1, dtype=torch.int64, device=device)
    correct, total, bad = counters[:K], counters[K:2 * K], counters[2 * K:]
    for images, labels in loader:
        ops.slice_argmax_count(engine.forward(images), cols_dev, labels, correct, total, bad)
    host = counters.cpu()                                    # the only host read of the task
    if int(host[2 * K]):
        raise IndexError("task %d: %d labels outside [0, %d)" % (task_idx + 1, int(host[2 * K]), K))
    accuracy = float(host[:K].sum()) * 100 / float(host[K:2 * K].sum())
    print("Accuracy: " + str(accuracy))
    if per_class_stats:
        return accuracy, host[:K].clone(), host[K:2 * K].clone()
    return accuracy
