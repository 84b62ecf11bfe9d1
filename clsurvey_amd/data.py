"""Device-resident task data.

The reference trains on pickled ImageFolder datasets that re-decode 8000 JPEGs per epoch through
8 DataLoader workers (EWC/main_EWC.py:28-31, data/imgfolder.py:86-128).  The framework uses the
raw, un-augmented sets (framework/main.py:197-202), so a whole Tiny-ImageNet task is a static
393 MB tensor: here it lives in HBM once and batches are gathered on device.

`DeviceLoader` reproduces the batch composition of torch's DataLoader(shuffle=True) bit for bit
for the same global torch RNG state (it consumes the global generator exactly like
_BaseDataLoaderIter.__init__ + RandomSampler.__iter__ do), so accuracy traces can be compared with
the reference run under the same seed (utilities/utils.py:52-58).
"""
import torch
from torch.utils.data import Dataset


class TensorTaskDataset(Dataset):
    """One split of one task. `classes` mirrors ImageFolder_Subset.classes (data/imgfolder.py)."""

    def __init__(self, x, y, classes):
        assert x.shape[0] == y.shape[0]
        self.x = x.contiguous().float()
        self.y = y.contiguous().long()
        self.classes = list(classes)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.y[i]


_TASK_CACHE = {}          # (path, mtime_ns, size, device) -> {'train' / 'val' / 'test': TensorTaskDataset in HBM}
_TASK_CACHE_BYTES = [0]


def load_task_datasets(dataset_path, device="cuda"):
    """torch.load(dataset_path) as every fine_tune_* entry point of the reference does (EWC/main_EWC.py:28), but the decoded
    task stays in HBM between calls: the framework opens the same 0.5 GB task file once per LR-grid node and per
    hyper-parameter decay attempt (~8x per task), which was ~40 % of a sweep's wall-clock.  Keyed by path + mtime + size;
    bounded by CLHIP_DATA_CACHE_GB (default 64, of 288 GB HBM), oldest entries dropped first.  A dict passes through."""
    import os
    if not isinstance(dataset_path, str):
        return dataset_path
    st = os.stat(dataset_path)
    key = (os.path.abspath(dataset_path), st.st_mtime_ns, st.st_size, str(device))
    hit = _TASK_CACHE.get(key)
    if hit is not None:
        return hit
    dsets = torch.load(dataset_path, weights_only=False)
    if not isinstance(dsets, dict) or not torch.cuda.is_available():
        return dsets
    out, nbytes = {}, 0
    for split, dset in dsets.items():
        x, y = _extract(dset)
        out[split] = TensorTaskDataset(x.to(device), y.to(device), getattr(dset, "classes", []))
        nbytes += x.numel() * 4 + y.numel() * 8
    limit = float(os.environ.get("CLHIP_DATA_CACHE_GB", "64")) * 2 ** 30
    while _TASK_CACHE and _TASK_CACHE_BYTES[0] + nbytes > limit:
        old = next(iter(_TASK_CACHE))
        _TASK_CACHE_BYTES[0] -= sum(d.x.numel() * 4 + d.y.numel() * 8 for d in _TASK_CACHE.pop(old).values())
    if nbytes <= limit:
        _TASK_CACHE[key] = out
        _TASK_CACHE_BYTES[0] += nbytes
    return out


def _extract(dataset):
    """(x, y) tensors of any map-style dataset (fast path for TensorTaskDataset)."""
    if isinstance(dataset, TensorTaskDataset):
        return dataset.x, dataset.y
    xs, ys = [], []
    for i in range(len(dataset)):
        item = dataset[i]
        xs.append(torch.as_tensor(item[0]))
        ys.append(int(item[1]))
    return torch.stack(xs).float(), torch.tensor(ys, dtype=torch.int64)


class DeviceLoader:
    """Iterates (x, y) batches of a dataset held in HBM. Same length / order semantics as
    torch.utils.data.DataLoader(dataset, batch_size, shuffle, drop_last=False)."""

    def __init__(self, dataset, batch_size, shuffle, device="cuda"):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.device = torch.device(device)
        x, y = _extract(dataset)
        self.x = x.to(self.device)
        self.y = y.to(self.device)
        self.n = self.x.shape[0]

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def order(self):
        # _BaseDataLoaderIter.__init__ draws the worker base seed first ...
        torch.empty((), dtype=torch.int64).random_()
        if not self.shuffle:
            return None
        # ... then RandomSampler.__iter__ seeds a private generator from the global one
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(self.n, generator=g)

    def __iter__(self):
        perm = self.order()
        if perm is not None:
            perm = perm.to(self.device)
        for s in range(0, self.n, self.batch_size):
            if perm is None:
                yield self.x[s:s + self.batch_size], self.y[s:s + self.batch_size]
            else:
                idx = perm[s:s + self.batch_size]
                yield self.x.index_select(0, idx), self.y.index_select(0, idx)


class TaskList(Dataset):
    """Several tasks as ONE dataset without a merged copy (data/imgfolder.py:244-272 ConcatDatasetDynamicLabels): it holds
    references to the per-task tensors `load_task_datasets` caches, labels of task j are shifted by the class counts of the
    tasks before it, global sample number -> (task, row) as torch's ConcatDataset does it (first task whose cumulative
    size exceeds the number)."""

    def __init__(self, dsets, classes_len=None):
        import itertools
        self.datasets = list(dsets)
        assert self.datasets, "TaskList needs at least one task"
        classes_len = [len(d.classes) for d in self.datasets] if classes_len is None else list(classes_len)
        self.cumulative_sizes = list(itertools.accumulate(len(d) for d in self.datasets))
        self.cumulative_classes_len = list(itertools.accumulate(classes_len))
        self.label_shifts = [0] + self.cumulative_classes_len[:-1]
        self.classes = [c for d in self.datasets for c in d.classes]

    def __len__(self):
        return self.cumulative_sizes[-1]

    def locate(self, idx):
        """int64 tensor of global sample numbers -> (task, local row, label shift) tensors; IndexError outside [0, len)."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError("TaskList: sample number outside [0, %d)" % len(self))
        cum = torch.tensor(self.cumulative_sizes, dtype=torch.int64)
        task = torch.bucketize(idx, cum, right=True)
        start = torch.cat([torch.zeros(1, dtype=torch.int64), cum[:-1]])
        return task, idx - start[task], torch.tensor(self.label_shifts, dtype=torch.int64)[task]

    def __getitem__(self, i):
        task, row, shift = (int(v) for v in self.locate([int(i)]))
        x, y = self.datasets[task][row]
        return x, y + shift


class MultiTaskLoader(DeviceLoader):
    """DeviceLoader over a TaskList: same length, order and consumption of the global RNG, but a batch is gathered straight
    out of the per-task tensors (clhip_gather_tasks) — the merged copy `ConcatTasks` makes (a second copy in HBM of every
    task the cache already holds) is never built."""

    def __init__(self, dataset, batch_size, shuffle, device="cuda"):
        from . import ops
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.device = torch.device(device)
        self.n = len(dataset)
        xs = [d.x for d in dataset.datasets]
        ys = [d.y for d in dataset.datasets]
        self.row_shape = tuple(xs[0].shape[1:])
        assert all(tuple(x.shape[1:]) == self.row_shape for x in xs), "tasks of one sequence share the image shape"
        self.row_elems = int(xs[0][0].numel())
        self.x = xs[0][:0]                      # (row shape only: what engine_for reads; no memory)
        self.table = ops.task_table(xs, ys, dataset.cumulative_sizes, dataset.label_shifts, self.device)

    def __iter__(self):
        from . import ops
        perm = self.order()
        if perm is None:
            perm = torch.arange(self.n)
        self.dataset.locate(perm[[int(perm.argmin()), int(perm.argmax())]] if self.n else perm)   # host check, before any launch
        perm = perm.to(self.device)
        for s in range(0, self.n, self.batch_size):
            x, y = ops.gather_tasks(self.table, self.row_elems, perm[s:s + self.batch_size])
            yield x.view((x.shape[0],) + self.row_shape), y


def synthetic_task(n_train, n_val, n_test, n_classes, hw=64, seed=7, noise=1.0, device="cpu", kind="protos", blobs=None):
    """Learnable synthetic task, SURVEY §8d.

    kind="protos" (the generator every committed fixture was made with): one full-resolution Gaussian prototype per class
    (std 0.5) + white pixel noise of std `noise`.  Linearly separable at any noise the tests use: a trained model is ~99 %
    sure of every training image, so its Fisher diagonal is ~0 and a regulariser has nothing to hold on to.

    kind="blobs" (bench.py's sweeps): image-like and NOT separable — a class prototype is a coarse g x g colour pattern
    (std `amp`) shown at full size, disturbed by coarse noise (std `noise_lr`, per cell) and white pixel noise (std `noise`);
    with probability 1 - q an image shows the prototype of a uniformly drawn class instead of its own (overlapping classes),
    so the best possible top-1 accuracy is q + (1 - q) / n_classes whatever the model: accuracies saturate at a level the DATA
    sets (two trainings that differ by rounding end at the same accuracy), the predictive distribution of a trained model
    keeps its entropy and the Fisher diagonal / MAS importance stay well away from 0.  `blobs` = dict(g, amp, noise_lr, q)."""
    g = torch.Generator()
    g.manual_seed(seed)
    names = [str(c) for c in range(n_classes)]
    out = {}
    if kind == "protos":
        protos = torch.randn((n_classes, 3, hw, hw), generator=g) * 0.5
        for name, n in (("train", n_train), ("val", n_val), ("test", n_test)):
            y = torch.randint(0, n_classes, (n,), generator=g)
            x = protos[y] + noise * torch.randn((n, 3, hw, hw), generator=g)
            out[name] = TensorTaskDataset(x.to(device), y.to(device), names)
        return out
    if kind != "blobs":
        raise ValueError("synthetic_task: kind is 'protos' or 'blobs'")
    b = dict(BLOBS_DEFAULT)
    b.update(blobs or {})
    cells = int(b["g"])
    if hw % cells:
        raise ValueError("synthetic_task: hw must be a multiple of the coarse grid g")
    protos = torch.randn((n_classes, 3, cells, cells), generator=g) * float(b["amp"])
    for name, n in (("train", n_train), ("val", n_val), ("test", n_test)):
        y = torch.randint(0, n_classes, (n,), generator=g)
        other = torch.randint(0, n_classes, (n,), generator=g)
        shown = torch.where(torch.rand((n,), generator=g) < float(b["q"]), y, other)
        coarse = protos[shown] + float(b["noise_lr"]) * torch.randn((n, 3, cells, cells), generator=g)
        x = coarse.repeat_interleave(hw // cells, 2).repeat_interleave(hw // cells, 3)
        x = x + noise * torch.randn((n, 3, hw, hw), generator=g)
        out[name] = TensorTaskDataset(x.to(device), y.to(device), names)
    return out


BLOBS_DEFAULT = {"g": 8, "amp": 4.0, "noise_lr": 1.2, "q": 0.8}
