"""Rehearsal baselines on the HIP path — mirror of src/methods/rehearsal/model/baseline_rehearsal_partial_mem.py (Net) and
baseline_rehearsal_full_mem.py (the same class with full_mem_mode), the R-PM / R-FM yardsticks of GEM.

Every training batch of task t also carries n_append stored exemplars of the earlier tasks.  The reference runs one
forward / backward per exemplar chunk of every past task and one for the current batch (:205-247): t + 1 engine passes
per step at task t.  Here the exemplars are device tensors (the store), and a step of a plan without BatchNorm is

    clhip_rehearsal_assemble           current batch + ring-buffer update + exemplar gather, one launch
    clhip_net_loss_step_loss_segments  ONE forward / segmented CE / backward over [current batch | exemplar chunks]
    SGD                                one fused kernel over the parameter arena

with the sample plan (which exemplars, in which chunk order) drawn on the host exactly as the reference draws it and
copied to the device in one non-blocking copy.  A plan with BatchNorm normalises every chunk with its own batch
statistics, so it takes the segmented path instead: one loss_step per chunk in the reference's order, weighted
accumulation with clhip_axpy.

Frame mode (exemplar.py): the store holds the loader's frames, the ring update copies them by sample number, and the step's
exemplars get one fresh (top, left, flip) each, drawn on the host after the plan and applied by the assembly launch
(clhip_rehearsal_assemble_crop_flip in place of clhip_rehearsal_assemble; everything after it is the same).  With a byte
store (frame_norm) the launch is clhip_rehearsal_assemble_crop_flip_u8: byte ring rows, exemplars decoded as they are cropped.
With a RandomResizedCropFlip spec it is clhip_rehearsal_assemble_resized_crop_flip[_u8]: the exemplars are resampled in the launch.
With a RandomPadCropFlip spec (padded replay) it is clhip_rehearsal_assemble_pad_crop_flip[_u8]: the store holds the unpadded
frames and the exemplars are windows of their padded frames, one (top, left, flip, h, w) each.
"""
import random

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from .._lib import check
from ..data import DeviceLoader
from ..optim import SGD
from .exemplar import ExemplarNet, SharedRowDropout, _stream, compact_blocks, compute_offsets  # noqa: F401


def replace_head(model, n_outputs):
    """baseline_rehearsal_partial_mem.py:36-41: a FRESH n_outputs-way Linear (torch default init, global CPU generator)."""
    last = str(len(model.classifier._modules) - 1)
    model.classifier._modules[last] = nn.Linear(model.classifier._modules[last].in_features, n_outputs)
    return model


class _Order(DeviceLoader):
    """DeviceLoader.order() over n items without holding data: the DataLoader(shuffle=True) draws of the exemplar loader."""

    def __init__(self, n):
        self.n, self.shuffle = int(n), True


def sample_plan(t, n_append, observed_tasks, n_memories, chunk_size, filled=None, seeds=None):
    """The reference's exemplar draws for one observe_FT step at task index t (:191-234), on Python `random` and the
    global torch CPU generator.  Returns (counts, [(task, slots, chunks)]) with chunks = lists of slots in the order the
    exemplar DataLoader of that task yields them.  `filled[task]` (optional) = slots of the task ever written: a slot at
    or above it is a None path in the reference.  `seeds` (optional list) collects the worker base seed every exemplar
    DataLoader draws (and the reference hands to its workers)."""
    if not (t > 0 and n_append > 0):
        return [], []
    n_fixed = int(np.floor(n_append / t))
    counts = [n_fixed for _ in range(t)]
    for _ in range(n_append % t):
        counts[random.randint(0, t - 1)] += 1
    out = []
    for tt in range(t):
        past = observed_tasks[tt]
        cnt = counts[past]
        if cnt <= 0:
            continue
        if cnt > n_memories:
            raise ValueError("rehearsal: task %d needs %d distinct exemplars of a memory of %d (the reference's rejection "
                             "sampling would never end)" % (past, cnt, n_memories))
        slots = []
        while len(slots) < cnt:
            idx = random.randint(0, n_memories - 1)
            if idx not in slots:
                slots.append(idx)
        if filled is not None and max(slots) >= filled[past]:
            raise ValueError("rehearsal: exemplar slot %d of task %d was never filled (%d stored; the reference would "
                             "load a None path)" % (max(slots), past, filled[past]))
        if chunk_size <= 0:
            raise ValueError("rehearsal: exemplar chunk size %d (batch fully taken by exemplars)" % chunk_size)
        loader = _Order(cnt)
        perm = loader.order().tolist()
        if seeds is not None:
            seeds.append(loader.base_seed)
        ordered = [slots[i] for i in perm]
        out.append((past, slots, [ordered[s:s + chunk_size] for s in range(0, cnt, chunk_size)]))
    return counts, out


class RehearsalNet(SharedRowDropout, ExemplarNet):
    """baseline_rehearsal_{partial,full}_mem.Net.  The pickle carries the net, the counters and the stored rows of the
    observed tasks only.  Dropout: GEM's shared mask rows (:97-111), reset at every step."""

    _TRANSIENT_EXTRA = ("store_x", "store_y", "store_ext", "last_gather", "last_exemplar_params")
    last_gather = last_exemplar_params = None                        # host: the last step's store rows and their draws

    def __init__(self, model, n_outputs, n_tasks, nc_per_task, n_memories, lr, weight_decay=0.0, full_mem_mode=False,
                 batch_size=200, in_shape=(3, 64, 64), device="cuda", exemplar_transform=None, frame_shape=None,
                 frame_norm=None):
        self.net = model.to(device)
        self.device = torch.device(device)
        self.n_outputs, self.n_tasks = n_outputs, n_tasks
        self.full_mem_mode = bool(full_mem_mode)
        self.n_total_memories = n_memories * n_tasks                # [n_tasks][n_memories] rows
        # :48-51: full mode is one pool, all of it for the first task
        self.n_memories = self.n_total_memories if self.full_mem_mode else n_memories
        self.batch_size = batch_size
        self.in_shape = tuple(in_shape)
        self._init_frames(exemplar_transform, frame_shape, frame_norm)
        self.cum_nc_per_task = [sum(nc_per_task[:i + 1]) for i in range(len(nc_per_task))]
        self.observed_tasks, self.old_task, self.mem_cnt = [], -1, 0
        self.filled = [0] * n_tasks                                 # slots of each task written at least once
        self.n_append, self.chunk_size = 0, batch_size
        self.force_segmented = False                                 # tests: run the BatchNorm path on any plan
        self.last_path = None                                        # 'fused' | 'segmented' | None (no step yet)
        self._load_rows({})
        self._bind()
        self.init_setup(lr=lr, weight_decay=weight_decay)

    def init_setup(self, args=None, lr=None, weight_decay=None, n_append=None, chunk_size=None):
        """:70-79: fresh SGD(momentum 0.9) at every main() call; the step composition of this call
        (args.n_exemplars_to_append_per_batch exemplars in chunks of the reduced args.batch_size)."""
        if args is not None:
            lr, weight_decay = args.lr, args.weight_decay
            n_append = getattr(args, "n_exemplars_to_append_per_batch", 0)
            chunk_size = args.batch_size
        if n_append is not None:
            self.n_append = int(n_append)
        if chunk_size is not None:
            self.chunk_size = int(chunk_size)
        self.dropout_masks = {}
        self.opt = SGD(self.net.parameters(), lr, momentum=0.9, weight_decay=weight_decay)

    def _rows_state(self):
        rows = (max(self.observed_tasks) + 1) * self.n_memories if self.observed_tasks else 0
        state = {"_rows_x": self.store_x[:rows].clone(), "_rows_y": self.store_y[:rows].clone()}
        if self.exemplar_transform is not None:
            state["_rows_ext"] = self.store_ext[:rows].clone()
        return state

    def _load_rows(self, rows):
        n = self.n_total_memories
        self.store_x = torch.zeros((n,) + self.store_shape, dtype=self.store_dtype, device=self.device)
        self.store_y = torch.zeros((n,), dtype=torch.int64, device=self.device)
        if self.exemplar_transform is not None:
            self.store_ext = self._full_ext(n)                       # host [rows][2]: valid (h, w) of every stored frame
        if rows:
            self.store_x[:rows["_rows_x"].shape[0]].copy_(rows["_rows_x"])
            self.store_y[:rows["_rows_y"].shape[0]].copy_(rows["_rows_y"])
            if self.exemplar_transform is not None:
                self.store_ext[:rows["_rows_ext"].shape[0]].copy_(rows["_rows_ext"])

    def _row(self, task, slot):
        return task * self.n_memories + slot

    def _eval_dropout(self, n):
        self.net.train(False)
        super()._eval_dropout(n)

    # ------------------------------------------------------------------ memory (:140-186)
    def switch_task(self, t):
        """:140-167: new task t; the ring counter restarts; full mode shares the pool out among the observed tasks and
        keeps the first n_per_task rows of every task, compacted in place in ascending task order."""
        self.init_new_task(t)
        self.mem_cnt = 0
        if not self.full_mem_mode:
            return
        n_new = int(self.n_total_memories / len(self.observed_tasks))
        self.filled = [min(f, n_new) for f in self.filled]
        stores = (self.store_x, self.store_y) + (() if self.exemplar_transform is None else (self.store_ext,))
        compact_blocks(stores, self.n_memories, n_new, self.filled)
        self.n_memories = n_new

    def ring_update(self, t, B, source=None):
        """:170-186: the first eff rows of a B-row batch go to slots [mem_cnt, mem_cnt + eff) of task t; the counter wraps
        at n_memories.  Frame mode: their extents go to store_ext.  Returns (first store row, eff)."""
        if (t + 1) * self.n_memories > self.store_x.shape[0]:
            raise ValueError("rehearsal: task %d does not fit the exemplar store" % t)
        endcnt = min(self.mem_cnt + B, self.n_memories)
        eff = endcnt - self.mem_cnt
        row0 = self._row(t, self.mem_cnt)
        self.filled[t] = max(self.filled[t], endcnt)
        self.mem_cnt = 0 if endcnt == self.n_memories else endcnt
        if self.exemplar_transform is not None:
            self.store_ext[row0:row0 + eff] = self._source_ext(source, eff)
        return row0, eff

    def plan(self, t, seeds=None):
        return sample_plan(t, self.n_append, self.observed_tasks, self.n_memories, self.chunk_size, self.filled, seeds)

    def exemplar_params(self, gather, seeds):
        """Frame mode: host int32 [len(gather)][params_width], one (top, left, flip) (a resized spec: (top, left, h, w, flip); a
        padded one: (top, left, flip, h, w)) per gathered store row in gather order, over the rows' own extents; the generator is seeded with the base seed the plan's last exemplar loader drew anyway (`seeds`
        of plan()), so the global generator and Python `random` are consumed exactly as in crop mode.  No exemplars: no draws."""
        if not gather:
            return torch.zeros((0, self.params_width), dtype=torch.int32)
        return self.draw_exemplar_params(self.store_ext[torch.tensor(gather, dtype=torch.int64)], seeds[-1])

    # ------------------------------------------------------------------ the step (:125-253)
    def observe_FT(self, x, t, y, source=None):
        """One rehearsal step: returns device (loss, hits on the current batch).  source: the batch's BatchSource in frame
        mode (exemplar.batch_source(loader)), None in crop mode."""
        self._check_source(source)
        frames = self.exemplar_transform is not None
        self.net.train(True)
        self.reset_dropout_config()
        if t != self.old_task:
            self.switch_task(t)
        B = int(y.shape[0])
        ring_row0, eff = self.ring_update(t, B, source)
        seeds = []
        _, plan = self.plan(t, seeds)
        chunks = [(past, ch) for past, _, chs in plan for ch in chs]
        segs = [(0, B) + self._slice(t) + (1.0, 0)]                 # every segment is of kind 0: cross-entropy
        gather = []
        for past, ch in chunks:
            segs.append((B + len(gather), B + len(gather) + len(ch)) + self._slice(past) + (1.0 / len(chunks), 0))
            gather.extend(self._row(past, s) for s in ch)
        E, N = len(gather), B + len(gather)
        if N > self.batch_size:
            raise RuntimeError("rehearsal: step of %d rows > engine batch %d" % (N, self.batch_size))
        self.last_gather = list(gather)
        if frames:
            self.last_exemplar_params = self.exemplar_params(gather, seeds)
            gather_dev, segs_dev, params_dev = self._upload(gather, ops.loss_segment_rows(segs), self.last_exemplar_params)
            self._assemble(x, y, B, source.frames, source.idx, self.store_x, self.store_y, ring_row0, eff,
                           gather_dev if E else None, params_dev if E else None, self.x_mix, self.y_mix)
        else:
            gather_dev, segs_dev = self._upload(gather, ops.loss_segment_rows(segs))
            row_elems = int(np.prod(self.in_shape))
            check(_lib.lib().clhip_rehearsal_assemble(
                x.data_ptr(), y.data_ptr(), B, row_elems, self.store_x.data_ptr(), self.store_y.data_ptr(), self.store_x.shape[0],
                ring_row0, eff, gather_dev.data_ptr() if E else None, E, self.x_mix.data_ptr(), self.y_mix.data_ptr(), _stream()),
                "clhip_rehearsal_assemble")
        self._dropout(True)
        self.stats.zero_()
        xm, ym = self.x_mix[:N], self.y_mix[:N]
        if self._fused(N, len(segs)):
            loss = self.engine.loss_step_segments(xm, ym, segs_dev, len(segs), self.stats)[0].clone()
        else:
            loss = self._segmented(xm, ym, segs)
        self.opt.step()
        return loss, self.stats[1]

    def _segmented(self, xm, ym, segs):
        """The reference's order: every exemplar chunk (tasks ascending), then the current batch; one loss_step per
        segment with its class slice."""
        def one_pass(g):
            r0, r1, o, nc, sc, _ = segs[g]
            loss, _ = self.engine.loss_step(xm[r0:r1], ym[r0:r1], "ce_mean", True, self.stats if g == 0 else None,
                                            class_slice=(o, o + nc))
            return loss, sc
        return self._accumulate(list(range(1, len(segs))) + [0], one_pass)
