"""GEM on the HIP path — mirror of src/methods/rehearsal/model/gem.py (Net.observe / forward /
fill_buffer / manage_memory) with the exemplar ring buffer held as TENSORS in HBM.

The reference stores exemplar *paths* and re-decodes n_memories JPEGs for every past task on every
training batch (gem.py:233-235); here memory[t] is a device tensor and a past-task pass is
ceil(n_memories / batch) engine calls.  Gradients of a task are one contiguous row of G (the
ParamArena gradient is flat), the QP inputs come from ONE Gram-matrix pass and the tiny QP (quadprog's Goldfarb-Idnani)
runs on the device in float64 (clhip_gem_qp) — no host round trip per batch.

Frame mode (exemplar.py): memory[t] holds the loader's frames, fill_buffer copies them by sample number (the ring-only form of
clhip_rehearsal_assemble_crop_flip), and a past-task pass serves memory[t] through the augmented DeviceLoader, a fresh crop
and flip per exemplar per pass as gem.py:233-234 rebuilds its ImagePathlist with the train transform.  With a byte store
(frame_norm) memory[t] holds uint8 frames and the memory loader is one over a ByteTaskDataset: the ..._u8 crop gather decodes them.
With a RandomResizedCropFlip spec the memory loader carries it, so a past-task pass runs the loaders' resizing gather.
With a RandomPadCropFlip spec (padded replay) memory[t] holds the UNPADDED frames, fill_buffer is the ring-only form of
clhip_rehearsal_assemble_pad_crop_flip[_u8] (a crop larger than the frame is legal there) and the memory loader carries the
spec with its fill (bytes on a byte store), so a past-task pass runs the loaders' padded gather.
"""
import copy
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import check
from ..data import ByteTaskDataset, DeviceLoader, TensorTaskDataset, _respec
from ..optim import SGD
from .exemplar import ExemplarNet, SharedRowDropout, _stream, batch_source, compute_offsets  # noqa: F401  (compute_offsets: imported from here)


def extend_head(model, n_outputs):
    """gem.py:99-113: replace the head by an n_outputs-way Linear whose first rows are the old head."""
    last = str(len(model.classifier._modules) - 1)
    old = copy.deepcopy(model.classifier._modules[last])
    new = nn.Linear(old.in_features, n_outputs)
    with torch.no_grad():
        new.weight[:old.out_features].copy_(old.weight)
        new.bias[:old.out_features].copy_(old.bias)
    model.classifier._modules[last] = new
    return model


class GemNet(SharedRowDropout, ExemplarNet):
    """gem.Net (gem.py:83-387).  The pickle carries the wrapped net, the exemplar tensors (memory_x / memory_labels, whole)
    and the counters.  Dropout: one shared mask row per layer (gem.py:166-196), reset at every observe."""

    _TRANSIENT_EXTRA = ("G", "_gram_ws", "_qp_ws", "_gram", "_v", "_info", "_qp_bad", "host_qp")
    NARROW_ROWS = 16                 # rows of a Gram matrix the register-resident kernels of csrc/gem.hip take
    MAX_TASKS = 64                   # CLHIP_GEM_WIDE_MAX: 63 memory rows + the current gradient (csrc/gem_wide.hip)

    def __init__(self, model, n_outputs, n_tasks, nc_per_task, n_memories, lr, weight_decay=0.0, memory_strength=1.0,
                 batch_size=200, in_shape=(3, 64, 64), device="cuda", exemplar_transform=None, frame_shape=None, frame_norm=None):
        if n_tasks > self.MAX_TASKS:
            raise ValueError("GEM: n_tasks = %d, the Gram / QP / projection kernels take at most %d tasks (CLHIP_GEM_WIDE_MAX)"
                             % (n_tasks, self.MAX_TASKS))
        self.net = model.to(device)
        self.device = torch.device(device)
        self.n_outputs, self.n_tasks, self.n_memories = n_outputs, n_tasks, n_memories
        self.batch_size = batch_size
        self.in_shape = tuple(in_shape)
        self._init_frames(exemplar_transform, frame_shape, frame_norm)
        self.memory_x = torch.zeros((n_tasks, n_memories) + self.store_shape, dtype=self.store_dtype, device=self.device)
        self.memory_labels = torch.zeros((n_tasks, n_memories), dtype=torch.int64, device=self.device)
        if self.exemplar_transform is not None:                     # host: valid (h, w) of every stored frame
            self.memory_ext = self._full_ext(n_tasks * n_memories).view(n_tasks, n_memories, 2)
        self.cum_nc_per_task = [sum(nc_per_task[:i + 1]) for i in range(len(nc_per_task))]
        self.observed_tasks, self.old_task, self.mem_cnt = [], -1, 0
        self._bind()
        self.init_setup(lr=lr, weight_decay=weight_decay, memory_strength=memory_strength)

    def _bind(self):
        super()._bind(mix=False)
        self.G = torch.zeros((self.n_tasks, self.A.numel), dtype=torch.float32, device=self.device)   # gem.py:131
        L = _lib.lib()
        # a Gram matrix has at most n_tasks rows (the memory rows of the earlier tasks + the current gradient); sequences of up
        # to 16 tasks use the register-resident kernels only, longer ones the wide entries once more than 16 rows are live
        rows = max(self.NARROW_ROWS, self.n_tasks)
        ws = L.clhip_gem_gram_ws(self.NARROW_ROWS)
        if rows > self.NARROW_ROWS:
            ws = max(ws, L.clhip_gem_gram_wide_ws(rows))
        self._gram_ws = torch.zeros(ws, dtype=torch.uint8, device=self.device)
        self._qp_ws = torch.zeros(max(L.clhip_gem_qp_wide_ws(rows) if rows > self.NARROW_ROWS else 0, 16), dtype=torch.uint8,
                                  device=self.device)
        self._gram = torch.zeros(rows * rows, dtype=torch.float64, device=self.device)
        self._v = torch.zeros(rows, dtype=torch.float64, device=self.device)        # QP solution, stays on the device
        self._info = torch.zeros(2, dtype=torch.int32, device=self.device)          # {violated constraints, status}
        self._qp_bad = torch.zeros(1, dtype=torch.int32, device=self.device)        # sticky: solves that did not report 'ok'
        self.host_qp = None          # tests only: a host solver f(gram, t, rows, margin) -> v replaces the device QP

    def init_setup(self, args=None, lr=None, weight_decay=None, memory_strength=None):
        """gem.py:146-155: fresh SGD(momentum 0.9) and margin; called after construction and after torch.load."""
        if args is not None:
            lr, weight_decay, memory_strength = args.lr, args.weight_decay, args.memory_strength
        self.dropout_masks = {}                                                                   # gem.py:152
        self.opt = SGD(self.net.parameters(), lr, momentum=0.9, weight_decay=weight_decay)       # gem.py:153
        self.margin = memory_strength

    # ------------------------------------------------------------------ memory
    def fill_buffer(self, t, x, y, source=None):
        """gem.py:322-345 (ring buffer; exemplar tensors instead of paths).  Frame mode: the frames of the batch's first eff
        samples (source: its BatchSource), one launch."""
        self._check_source(source)
        bsz = y.shape[0]
        endcnt = min(self.mem_cnt + bsz, self.n_memories)
        eff = endcnt - self.mem_cnt
        if self.exemplar_transform is not None:
            self._assemble(None, y, bsz, source.frames, source.idx, self.memory_x.view((-1,) + self.frame_shape),
                           self.memory_labels.view(-1), t * self.n_memories + self.mem_cnt, eff, None, None, None, None)
            self.memory_ext[t, self.mem_cnt:endcnt] = self._source_ext(source, eff)
        else:
            self.memory_x[t, self.mem_cnt:endcnt] = x[:eff]
            self.memory_labels[t, self.mem_cnt:endcnt] = y[:eff]
        self.mem_cnt += eff
        if self.mem_cnt == self.n_memories:
            self.mem_cnt = 0
            return True
        return False

    def manage_memory(self, t, loader):
        """gem.py:347-368: fill the buffer from the first-task training set."""
        for x, y in loader:
            if t != self.old_task:
                self.init_new_task(t)
            if self.fill_buffer(t, x, y, batch_source(loader) if self.exemplar_transform is not None else None):
                return True
        return False

    def _memory_loader(self, past):
        """The shuffled loader of one past task's memory pass; frame mode: augmented with the stored frames' own extents."""
        mem = TensorTaskDataset.__new__(TensorTaskDataset) if self.frame_norm is None else ByteTaskDataset.__new__(ByteTaskDataset)
        mem.x, mem.y, mem.classes = self.memory_x[past], self.memory_labels[past], []
        if self.frame_norm is not None:
            mem.mean, mem.std = self.frame_norm                     # the ..._u8 crop gather decodes the stored bytes
        if self.exemplar_transform is not None:
            # (crop, resized or padded: the loader serves all three; a padded spec keeps its fill, bytes on a byte store)
            mem.transform = _respec(self.exemplar_transform, self.memory_ext[past])
        return DeviceLoader(mem, self.batch_size, True, self.device)

    # ------------------------------------------------------------------ kernels
    def _axpy(self, row, assign):
        check(_lib.lib().clhip_axpy(row.data_ptr(), self.A.grad.data_ptr(), self.A.numel, 1.0, int(assign), _stream()),
              "clhip_axpy")

    def gram(self, rows, to_host=True):
        m = len(rows)
        idx = (C.c_int * m)(*rows)
        L = _lib.lib()
        name = "clhip_gem_gram" if m <= self.NARROW_ROWS else "clhip_gem_gram_wide"
        check(getattr(L, name)(self.G.data_ptr(), self.G.shape[1], idx, m, self.A.numel, self._gram.data_ptr(),
                               self._gram_ws.data_ptr(), self._gram_ws.numel(), _stream()), name)
        return self._gram[:m * m].cpu().numpy().reshape(m, m) if to_host else self._gram

    def project_on_device(self, rows, t, eps=1e-3):
        """Violation test (gem.py:275-277), QP (:58-80) and projection / overwrite_grad (:79, :38-55) of the current
        gradient G[t] without a host round trip: Gram of rows + [t] -> clhip_gem_qp -> clhip_gem_project_dev.  Returns the
        device counter of violated constraints (0 => the gradient was left as it is)."""
        m = len(rows) + 1
        self.gram(list(rows) + [t], to_host=False)
        L = _lib.lib()
        idx = (C.c_int * (m - 1))(*rows)
        if m <= self.NARROW_ROWS:
            check(L.clhip_gem_qp(self._gram.data_ptr(), m, float(self.margin), float(eps), self._v.data_ptr(), self._info.data_ptr(),
                                 _stream()), "clhip_gem_qp")
            check(L.clhip_gem_project_dev(self.G.data_ptr(), self.G.shape[1], idx, self._v.data_ptr(), self._info.data_ptr(), m - 1,
                                          self.G[t].data_ptr(), self.A.grad.data_ptr(), self.A.numel, _stream()),
                  "clhip_gem_project_dev")
        else:                                    # more than 16 rows: the workgroup QP and the 63-row projection
            check(L.clhip_gem_qp_wide(self._gram.data_ptr(), m, float(self.margin), float(eps), self._v.data_ptr(),
                                      self._info.data_ptr(), self._qp_ws.data_ptr(), self._qp_ws.numel(), _stream()),
                  "clhip_gem_qp_wide")
            check(L.clhip_gem_project_dev_wide(self.G.data_ptr(), self.G.shape[1], idx, self._v.data_ptr(), self._info.data_ptr(),
                                               m - 1, self.G[t].data_ptr(), self.A.grad.data_ptr(), self.A.numel, _stream()),
                  "clhip_gem_project_dev_wide")
        self._qp_bad += self._info[1:2]          # status 1 (iteration limit) / 2 (infeasible) must not pass silently
        return self._info[0].clone()

    def check_qp_status(self):
        """Raise if any projection since the last call ended without a solution (the reference's quadprog raises in that
        batch; here the status is a device counter read once per epoch, no synchronisation per batch)."""
        bad = int(self._qp_bad.item())
        self._qp_bad.zero_()
        if bad:
            raise RuntimeError("GEM: project2cone2's QP reported iteration limit / infeasibility (status sum %d)" % bad)

    def project(self, rows, v, t):
        m = len(rows)
        idx = (C.c_int * m)(*rows)
        vv = (C.c_float * m)(*[float(a) for a in v])
        name = "clhip_gem_project" if m <= self.NARROW_ROWS else "clhip_gem_project_wide"
        check(getattr(_lib.lib(), name)(self.G.data_ptr(), self.G.shape[1], idx, vv, m, self.G[t].data_ptr(),
                                        self.A.grad.data_ptr(), self.A.numel, _stream()), name)

    # ------------------------------------------------------------------ gem.py:206-287
    def observe(self, x, t, y, source=None):
        batch_stats = {"projected_grads": [0]}
        if t != self.old_task:
            self.init_new_task(t)
        self.fill_buffer(t, x, y, source)
        self.reset_dropout_config()                                   # gem.py:214-215: net.train(); fresh masks per observe
        self._dropout(True)
        if len(self.observed_tasks) > 1:
            for past in self.observed_tasks[:-1]:
                sl = compute_offsets(past, self.cum_nc_per_task)
                first = True
                for xb, yb in self._memory_loader(past):
                    self.engine.loss_step(xb.contiguous(), yb.contiguous(), "ce_mean", True, class_slice=sl)
                    self._axpy(self.G[past], assign=first)          # grads accumulate over batches (:237-256)
                    first = False
        sl = compute_offsets(t, self.cum_nc_per_task)
        self.stats.zero_()
        loss, _ = self.engine.loss_step(x, y, "ce_mean", True, self.stats, class_slice=sl)
        loss = loss.clone()
        if len(self.observed_tasks) > 1:
            self._axpy(self.G[t], assign=True)                       # store_grad (:272)
            rows = list(self.observed_tasks[:-1]) + [t]
            if self.host_qp is None:
                batch_stats["projected_grads"] = [self.project_on_device(rows[:-1], t)]     # device counter, no sync
            else:                                                     # injected host solver (cross-check in the tests)
                gram = self.gram(rows)
                dotp = gram[-1, :-1]                                  # g . G_tt (:275-276)
                viol = int((dotp < 0).sum())
                if viol != 0:
                    batch_stats["projected_grads"] = [viol]
                    v = self.host_qp(gram, len(rows) - 1, list(range(len(rows) - 1)), self.margin)
                    self.project(rows[:-1], v, t)                     # project2cone2 + overwrite_grad (:278-283)
        self.opt.step()
        return loss, self.stats[1], batch_stats

    def observe_FT(self, x, t, y, source=None):
        """gem.py:289-309: plain SGD step on the task's output slice (phase-1 grid; no memory)."""
        self._check_source(source)
        sl = compute_offsets(t, self.cum_nc_per_task)
        self.stats.zero_()
        self._dropout(True)       # no reset here: the masks drawn after init_setup stay for the whole run, as in the reference
        loss, _ = self.engine.loss_step(x, y, "ce_mean", True, self.stats, class_slice=sl)
        self.opt.step()
        return loss, self.stats[1]
