"""What the exemplar methods (GEM, the rehearsal baselines R-PM / R-FM, iCaRL) share on the HIP path: a wrapper around a
net and its NetEngine that pickles like the reference's nn.Module, evaluates on a task's slice of the shared head, and runs
a training step over [current batch | exemplar chunks] either as ONE fused pass (clhip_net_loss_step_loss_segments) or,
for a plan with BatchNorm or a step over the loss kernel's limits, segment by segment with clhip_axpy accumulation.

A method derives from ExemplarNet and one of the two dropout policies and keeps what is its own: the store layout, the
host draws, the memory management and the composition of its step.
"""
import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from ..net import NetEngine

FUSED_MAX_ROWS, FUSED_MAX_SEGS = ops.LOSS_MAX_ROWS, ops.LOSS_MAX_SEGS        # the fused loss's limits (include/clhip.h)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def compute_offsets(task_idx, cum_nc_per_task):
    """rehearsal/model/common.py:106-118."""
    o1 = 0 if task_idx == 0 else int(cum_nc_per_task[task_idx - 1])
    return o1, int(cum_nc_per_task[task_idx])


def compact_blocks(tensors, old_stride, new_stride, keep_per_block):
    """Block k of every tensor moves from row k * old_stride to row k * new_stride (new_stride <= old_stride) and keeps its
    first keep_per_block[k] rows; in place, ascending: a destination never overtakes its source, and pieces no longer than
    the gap mean that no piece overlaps its own source."""
    for k, keep in enumerate(keep_per_block):
        src, dst = k * old_stride, k * new_stride
        gap = src - dst
        s = 0
        while gap > 0 and s < keep:
            e = min(keep, s + gap)
            for t in tensors:
                t[dst + s:dst + e] = t[src + s:src + e]
            s = e


class SharedRowDropout:
    """GEM's manual dropout (gem.py:166-196, baseline_rehearsal_partial_mem.py:97-111): in training mode every Dropout of the
    plan multiplies its input by ONE mask row Bernoulli(p_retain) / p_retain of a single sample's shape, drawn (device
    generator) when first needed after a reset and shared by all samples and passes until the next reset; p_retain is the
    fixed 0.5 of the reference's signature, not module.p.  Eval: identity."""

    _TRANSIENT_POLICY = ("dropout_masks", "_draw_mask")

    def _bind(self, *args, **kw):
        super()._bind(*args, **kw)
        self.dropout_masks = {}

    def reset_dropout_config(self):
        self.dropout_masks = {}

    def _dropout(self, train, p_retain_unit=0.5):
        for li in self.engine.drops:
            if not train:
                self.engine.set_dropout(li, None)
                continue
            if li not in self.dropout_masks:
                self.dropout_masks[li] = self._draw_mask(li, self.engine.in_elems[li], p_retain_unit)
            self.engine.set_dropout(li, self.dropout_masks[li])

    def _draw_mask(self, layer, n, p_retain_unit):
        """torch.bernoulli(fill(p_retain)) / p_retain over one sample's features."""
        return torch.full((n,), p_retain_unit, dtype=torch.float32, device=self.device).bernoulli_().div_(p_retain_unit)

    def _eval_dropout(self, n):
        self._dropout(False)


class PerRowDropout:
    """nn.Dropout of the wrapped net: while net.training, a fresh Bernoulli(1 - p) / (1 - p) mask per element and row for
    every pass (device generator); identity in eval mode."""

    _TRANSIENT_POLICY = ("_draw_mask",)

    def _dropout(self, n):
        """Masks of one pass over n rows, or none in eval mode.  Returns {layer: mask}."""
        masks = {}
        for li, m in self.engine.drops.items():
            if self.net.training and m.p > 0:
                masks[li] = self._draw_mask(li, n, self.engine.in_elems[li], m.p)
                self.engine.set_dropout(li, masks[li])
            else:
                self.engine.set_dropout(li, None)
        return masks

    def _draw_mask(self, layer, n, elems, p):
        keep = 1.0 - p
        return torch.empty((n, elems), dtype=torch.float32, device=self.device).bernoulli_(keep).div_(keep)

    def _eval_dropout(self, n):
        self.net.train(False)
        self._dropout(n)


class ExemplarNet:
    """Picklable like the reference's nn.Module (torch.save(model) / copy.deepcopy(model) in train_rehearsal.py:176-180): the
    pickle carries the wrapped net, the counters and what _rows_state() returns of the store; engine / workspaces /
    optimizer are rebuilt on load (_bind, then the trainer's init_setup)."""

    _TRANSIENT = ("engine", "A", "stats", "opt", "x_mix", "y_mix", "_acc")
    _TRANSIENT_POLICY = ()          # the dropout policy's state
    _TRANSIENT_EXTRA = ()           # the subclass's own device state

    def _bind(self, mix=True):
        """Engine and work buffers; mix: the [current batch | exemplar chunks] rows of a step."""
        rows = max(self.batch_size, 1)
        self.engine = NetEngine(self.net, rows, self.in_shape, self.device)
        self.engine.auto_dropout = False        # the masks are the wrapper's own (its dropout policy), not the engine's
        self.A = self.engine.arena
        self.stats = torch.zeros(2, dtype=torch.float64, device=self.device)
        if mix:
            self.x_mix = torch.empty((rows,) + self.in_shape, dtype=torch.float32, device=self.device)
            self.y_mix = torch.empty((rows,), dtype=torch.int64, device=self.device)
            self._acc = None

    def _rows_state(self):
        """Hook: {'_rows_x': ..., ...}, copies of the store rows in use (a view would pickle the whole store)."""
        return {}

    def _load_rows(self, rows):
        """Hook: rebuild the store from what _rows_state() returned."""

    def __getstate__(self):
        transient = self._TRANSIENT + self._TRANSIENT_POLICY + self._TRANSIENT_EXTRA
        state = {k: v for k, v in self.__dict__.items() if k not in transient}
        state.update(self._rows_state())
        return state

    def __setstate__(self, state):
        rows = {k: state.pop(k) for k in [k for k in state if k.startswith("_rows_")]}
        self.__dict__.update(state)
        self.device = torch.device(self.device)
        self.net = self.net.to(self.device)
        self._load_rows({k: v.to(self.device) for k, v in rows.items()})
        self._bind()
        self.opt = None

    def compute_offsets(self, task_idx, cum_nc_per_task=None):
        return compute_offsets(task_idx, self.cum_nc_per_task if cum_nc_per_task is None else cum_nc_per_task)

    def _slice(self, task):
        o1, o2 = compute_offsets(task, self.cum_nc_per_task)
        return (o1, o2 - o1)

    def parameters(self):
        return self.net.parameters()

    def eval(self):
        return self

    def to(self, device):
        return self

    def init_new_task(self, t):
        self.observed_tasks.append(t)
        self.old_task = t

    # ------------------------------------------------------------------ the step over [current batch | exemplar chunks]
    def _upload(self, gather, rows):
        """Gather rows (int32) and rows of int32 columns (clhip_loss_segment tables: ops.loss_segment_rows) in ONE pinned
        host buffer, one non-blocking copy.  Returns the two device parts, the second one flat."""
        pinned = torch.empty(len(gather) + rows.size, dtype=torch.int32, pin_memory=True)
        host = pinned.numpy()
        host[:len(gather)] = gather
        host[len(gather):] = rows.reshape(-1)
        dev = pinned.to(self.device, non_blocking=True)     # the caching host allocator keeps `pinned` until the copy ran
        return dev[:len(gather)], dev[len(gather):]

    def _fused(self, N, n_segs):
        """One fused pass, or segment by segment: a plan with BatchNorm normalises every chunk with its own statistics, and
        the fused loss takes FUSED_MAX_ROWS rows and FUSED_MAX_SEGS segments (a late task with a big batch, or a chunk
        size near 1, goes over them)."""
        fused = not (self.engine.bns or self.force_segmented or N > FUSED_MAX_ROWS or n_segs > FUSED_MAX_SEGS)
        self.last_path = "fused" if fused else "segmented"
        return fused

    def _accumulate(self, order, one_pass):
        """The segmented path: one_pass(g) runs forward / loss / backward of segment g and returns (loss[1], factor); the
        gradients are summed as sum_g factor_g * grad_g (clhip_axpy) into the arena.  Returns the summed loss."""
        if self._acc is None:
            self._acc = torch.empty(self.A.numel, dtype=torch.float32, device=self.device)
        total = torch.zeros(1, dtype=torch.float32, device=self.device)
        for k, g in enumerate(order):
            loss, sc = one_pass(g)
            total += loss if sc == 1.0 else loss * sc
            check(_lib.lib().clhip_axpy(self._acc.data_ptr(), self.A.grad.data_ptr(), self.A.numel, float(sc), int(k == 0),
                                        _stream()), "clhip_axpy")
        self.A.grad.copy_(self._acc)
        return total

    # ------------------------------------------------------------------ evaluation on a task's slice of the head
    def eval_batch(self, x, y, t, stats):
        """main_rehearsal.py:18-35: CE and hits on the task slice (accumulated into stats on the device)."""
        self._eval_dropout(x.shape[0])
        return self.engine.loss_step(x, y, "ce_mean", False, stats, class_slice=compute_offsets(t, self.cum_nc_per_task))[0]

    def _mask_slice(self, logits, t):
        """logits with everything outside task t's slice at -10e10."""
        o1, o2 = compute_offsets(t, self.cum_nc_per_task)
        res = torch.full_like(logits, -10e10)
        res[:, o1:o2] = logits[:, o1:o2]
        return res

    def __call__(self, x, t, **kw):
        return self.forward(x, t)

    def forward(self, x, t):
        """Eval mode: logits with everything outside the task slice at -1e11."""
        self._eval_dropout(x.shape[0])
        return self._mask_slice(self.engine.forward(x), t)
