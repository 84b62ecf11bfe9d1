"""iCaRL on the HIP path — mirror of src/methods/rehearsal/model/icarl.py (Net.manage_memory / update_representation /
forward), the survey's variant: one total memory shared out per class (K/m), distillation per past task, nearest-mean-of-
exemplars evaluation inside the task's slice.

The reference stores exemplar *paths* and, to rank the exemplars of one class, recomputes the features of every class
image and of every exemplar chosen so far once per pick (:394-427).  Here the exemplars are device tensors (the store) and

    manage_memory   features of the task's training set ONCE (chunks through the plan, NetEngine.layer_input of the first
                    Linear layer), then clhip_icarl_herd: the ranked lists of all classes of the task in one launch
    observe         host draws exactly as the reference makes them, clhip_rehearsal_assemble (images; a second launch
                    gathers the stored distillation rows), then ONE clhip_net_loss_step_loss_segments over
                    [current batch | distillation chunks] and one fused SGD step
    forward         class means from the stored exemplars once per (model, task), clhip_icarl_nme per batch

A plan with BatchNorm, or a step over the loss kernel's limits, takes the segmented path: one pass per chunk in the
reference's order (as RehearsalNet does).  Herding needs features that do not depend on the batch: manage_memory refuses a
net with BatchNorm in `features`.

Frame mode (a wrapper built with exemplar_transform, exemplar.py): iCaRL on AUGMENTED tasks.  The reference's memory holds
paths; under a random train transform every replay is a fresh crop (:560-561) while the distillation targets stay the rows
computed once at herding time on the crop the winner had then (:476-479).  Here

    store           store_x holds the winners' FRAMES (fp32, or bytes with frame_norm), store_ext (host) their valid (h, w),
                    store_t their distillation rows; all three move together through _truncate
    manage_memory   the HERDING VIEW: one draw of the train transform per training image, dataset order, over the split's own
                    extents, private CPU generator seeded view_seed_of(view_seed, t, VIEW_HERD); features once on those crops
                    (the loaders' gathers over a one-task table, chunks of the engine's batch), ranking and K_c as above;
                    store_t = forward_training of the winners' herding-view crops
    observe         a fresh draw per gathered exemplar (draw_exemplar_params over store_ext, seeded with the base seed the plan's
                    last exemplar loader drew anyway: the global generators are consumed as in crop mode), then ONE
                    clhip_icarl_assemble_* launch: current rows, exemplar windows, label 0, target rows -> x_mix, y_mix, t_mix
    class_means     the CLASS-MEAN VIEW: one draw per stored exemplar, seed kind VIEW_MEANS, cropped by the same entry with B = 0

Seed rule: view_seed_of(view_seed, t, kind) = (view_seed * 1000003 + t) * 2 + kind, nothing else; view_seed is a wrapper
attribute (default 0, pickled).  Neither view touches the global torch generator, numpy or Python `random`.
What differs from the reference: its manage_memory runs the class loader once per pick (:394-451), so with a random transform
the mean, the costs of every pick and the stored target each see other crops of the images; the herding view is that procedure
with the loader's draws frozen over the passes.  Its forward redraws the exemplars' crops for every evaluated batch (:160-167);
the class-mean view is one draw per (model, task, batch size), so an evaluation is reproducible.  Without freedom (frames of
the crop size, p = 0) frame mode is bitwise crop mode.

Padded frame mode (exemplar_transform a RandomPadCropFlip: RandomCrop(size, padding, fill, padding_mode) + flip, the CIFAR-style
rule): the store holds the UNPADDED frames and store_ext their valid extents; a draw is (top, left, flip, h, w) with the corner in
the frame's unpadded coordinates (>= -pad).  The two views gather through ops.gather_tasks_pad_crop_flip[_u8], the step and the
class-mean view through clhip_icarl_assemble_pad_crop_flip[_u8], all with (padding_mode, padding, self.fill); fill is the device
float[C] of the output domain that _bind rebuilds (a byte fill decoded through the table on a byte store).  Bitwise the crop-frame
wrapper on the same frames padded on the host.  pad_if_needed is not built.
"""
import random

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from ..data import ByteTaskDataset, RandomPadCropFlip, RandomResizedCropFlip, _spec_key, _transform_of
from ..optim import SGD
from .exemplar import BatchSource, ExemplarNet, PerRowDropout, _stream, compact_blocks, compute_offsets
from .gem import extend_head
from .rehearsal import _Order

T_DISTILL = 2.0                 # update_representation(..., T=2)
HERD_MAX_FEATS = 16384          # CLHIP_ICARL_MAX_FEATS_WIDE (include/clhip.h): ops.icarl_herd picks the entry by width


def init_head(model, n_outputs):
    """icarl.py:84-103: an n_outputs-way Linear whose first rows are the old head."""
    return extend_head(model, n_outputs)


def mean_weights(n, batch_size):
    """Per-row weights of get_mean_feat (:303-311) over n rows in order, batches of batch_size: the mean of batch means
    is sum_i w_i f_i with w_i = 1 / (n_batches * size of i's batch) — a short last batch weighs more per row."""
    n_batches = (n + batch_size - 1) // batch_size
    w = np.empty(n, dtype=np.float32)
    for b in range(n_batches):
        lo, hi = b * batch_size, min(n, (b + 1) * batch_size)
        w[lo:hi] = 1.0 / (n_batches * (hi - lo))
    return w


VIEW_HERD, VIEW_MEANS = 0, 1     # the two private draws of a frame-mode wrapper (view_seed_of's `kind`)


def view_seed_of(view_seed, t, kind):
    """Seed of the private CPU generator that draws a view of task t: the herding view (kind VIEW_HERD, one draw of the train
    transform per training image at manage_memory) or the class-mean view (VIEW_MEANS, one per stored exemplar at class_means).
    A function of (view_seed, t, kind) alone: (view_seed * 1000003 + t) * 2 + kind."""
    return (int(view_seed) * 1000003 + int(t)) * 2 + int(kind)


def exemplar_draws(t, n_append, class_len, exemplar_count, nc_per_task, cum_nc_per_task, total_batch_size, seeds=None):
    """The host draws of update_representation (:507-562) for one step at task index t, on Python `random`, numpy's global
    generator and the global torch CPU generator, in the reference's order.  class_len[c] = exemplars stored for class c
    (every class stored so far).  Returns (counts per class, [(task, chunks)]) with chunks = lists of (class, exemplar
    index) in the order the task's DataLoader(shuffle=True, batch_size=total_batch_size) yields them.  `seeds` (optional list)
    collects the worker base seed every exemplar DataLoader draws (rehearsal.sample_plan's rule); the draws are the same with or
    without it."""
    n_classes = len(class_len)
    if exemplar_count <= 0 or n_classes == 0:
        return [], []
    n_fixed = int(np.floor(n_append / n_classes))
    if n_fixed > exemplar_count:                       # :511-513: capped, no random leftovers
        counts = [exemplar_count] * n_classes
    else:
        counts = [n_fixed] * n_classes
        n_random = n_append % n_classes
        if n_random > sum(exemplar_count - c for c in counts):
            raise ValueError("icarl: %d leftover exemplars do not fit %d classes of %d (the reference's redraw loop would "
                             "never end)" % (n_random, n_classes, exemplar_count))
        rnd = 0
        while rnd < n_random:
            idx = random.randint(0, n_classes - 1)
            if counts[idx] < exemplar_count:
                counts[idx] += 1
                rnd += 1
    out = []
    for task in range(t):
        o1, _ = compute_offsets(task, cum_nc_per_task)
        rows = []
        for local in range(nc_per_task[task]):
            c = local + o1
            if c < n_classes and counts[c] > 0:
                picks = np.random.permutation(class_len[c])[:counts[c]].tolist()
                rows.extend((c, int(e)) for e in picks)
        if not rows:
            continue
        if total_batch_size <= 0:
            raise ValueError("icarl: distillation chunk size %d" % total_batch_size)
        loader = _Order(len(rows))
        ordered = [rows[i] for i in loader.order().tolist()]
        if seeds is not None:
            seeds.append(loader.base_seed)
        out.append((task, [ordered[s:s + total_batch_size] for s in range(0, len(ordered), total_batch_size)]))
    return counts, out


def segment_scales(chunk_counts, reg):
    """The accumulation of :505-592 AS WRITTEN: total_ex_loss and its counter are not reset between past tasks and
    reg * total / count is added once per past task.  With A_j the sum of task j's chunk losses and c_j its chunk count:
    T_1 = reg A_1 / c_1, T_j = reg (T_{j-1} + A_j) / (c_1 + ... + c_j), loss += sum_j T_j.  Linear in the chunk losses:
    returns the factor of one chunk loss of each task (same order as chunk_counts)."""
    n = len(chunk_counts)
    coef = [0.0] * n                  # factor of A_i inside the running total
    scale = [0.0] * n
    count = 0
    for j in range(n):
        count += chunk_counts[j]
        coef[j] += 1.0
        coef = [reg * c / count for c in coef[:j + 1]] + coef[j + 1:]
        for i in range(j + 1):
            scale[i] += coef[i]
    return scale


class IcarlNet(PerRowDropout, ExemplarNet):
    """icarl.Net.  The pickle carries the net, the counters, the stored exemplar rows and their distillation targets only.
    Dropout: the net's own nn.Dropout, one mask per step over the MIXED batch."""

    _TRANSIENT_EXTRA = ("t_mix", "store_x", "store_t", "_store_lab", "_means", "_scratch_lab", "last_ranking", "store_ext",
                        "last_gather", "last_exemplar_params", "last_herd_params")
    view_seed = 0                                                    # class-level default: an older pickle loads with 0
    last_gather = last_exemplar_params = last_herd_params = None     # host: the last step's store rows and draws, the last herding view

    def __init__(self, model, n_outputs, n_tasks, nc_per_task, n_memories, lr, weight_decay=0.0, memory_strength=0.0,
                 batch_size=200, in_shape=(3, 64, 64), device="cuda", exemplar_transform=None, frame_shape=None,
                 frame_norm=None):
        self.net = init_head(model, n_outputs).to(device)
        self.device = torch.device(device)
        self.n_outputs, self.n_tasks = n_outputs, n_tasks
        self.n_memories_per_task = int(n_memories)
        self.n_total_memories = int(n_memories) * n_tasks            # :41, fixed at creation
        self.batch_size = batch_size
        self.in_shape = tuple(in_shape)
        self._init_frames(exemplar_transform, frame_shape, frame_norm)
        if self.exemplar_transform is not None:                      # (a crop-mode wrapper draws no view: its pickle keeps its keys)
            self.view_seed = 0                                       # seeds the herding and class-mean views (view_seed_of)
        self.nc_per_task = list(nc_per_task)
        self.cum_nc_per_task = [sum(nc_per_task[:i + 1]) for i in range(len(nc_per_task))]
        self.exemplar_count = 0          # K/m of the last manage_memory = the row stride of a class block in the store
        self.class_len = []              # exemplars stored per class, classes in head order
        self.observed_tasks, self.old_task = [], -1
        self.n_append, self.chunk_size, self.total_batch_size = 0, batch_size, batch_size
        self.force_segmented = False                                 # tests: run the BatchNorm path on any plan
        self.last_path = None                                        # 'fused' | 'segmented' | None (no observe yet)
        self._load_rows({})
        self._bind()
        self.init_setup(lr=lr, weight_decay=weight_decay, memory_strength=memory_strength)

    # ------------------------------------------------------------------ state
    def _bind(self):
        super()._bind()
        self.fc_first = next(i for i, sp in enumerate(self.engine.layers) if sp[0] == "fc")
        rows = self.engine.max_batch
        self.t_mix = torch.zeros((rows, self.n_outputs), dtype=torch.float32, device=self.device)
        self._scratch_lab = torch.empty((rows,), dtype=torch.int64, device=self.device)
        self._means = {}
        self.last_ranking = None      # (device int32 ranking, class offsets) of the last manage_memory; not pickled

    def init_setup(self, args=None, lr=None, weight_decay=None, memory_strength=None, n_append=None, chunk_size=None,
                   total_batch_size=None):
        """:105-124: fresh SGD(momentum 0.9) and reg at every main() call; the step composition of this call."""
        if args is not None:
            lr, weight_decay, memory_strength = args.lr, args.weight_decay, args.memory_strength
            n_append = getattr(args, "n_exemplars_to_append_per_batch", 0)
            chunk_size = args.batch_size
            total_batch_size = getattr(args, "total_batch_size", args.batch_size)
            if args.n_outputs != self.n_outputs:
                raise NotImplementedError("icarl: the head is sized for every task at creation (%d outputs, asked %d)"
                                          % (self.n_outputs, args.n_outputs))
            if args.n_tasks != self.n_tasks:
                self.n_tasks = args.n_tasks                        # :115-119: the memory keeps its initial capacity
            self.nc_per_task = list(args.nc_per_task)
            self.cum_nc_per_task = [sum(self.nc_per_task[:i + 1]) for i in range(len(self.nc_per_task))]
        if n_append is not None:
            self.n_append = int(n_append)
        if chunk_size is not None:
            self.chunk_size = int(chunk_size)
        if total_batch_size is not None:
            self.total_batch_size = int(total_batch_size)
        self.opt = SGD(self.net.parameters(), lr, momentum=0.9, weight_decay=weight_decay)
        if memory_strength is not None:
            self.reg = memory_strength

    def _block(self, c):
        """(first store row, length) of class c."""
        return c * self.exemplar_count, self.class_len[c]

    def stored_rows(self):
        """Store rows that hold an exemplar, class after class."""
        return [c * self.exemplar_count + e for c in range(len(self.class_len)) for e in range(self.class_len[c])]

    def _rows_state(self):
        idx = torch.tensor(self.stored_rows(), dtype=torch.int64, device=self.device)
        state = {"_rows_x": self.store_x.index_select(0, idx), "_rows_t": self.store_t.index_select(0, idx)}
        if self.exemplar_transform is not None:
            state["_rows_ext"] = self.store_ext.index_select(0, idx.cpu())
        return state

    def _load_rows(self, rows):
        n = self.n_total_memories
        self.store_x = torch.zeros((n,) + self.store_shape, dtype=self.store_dtype, device=self.device)
        if self.exemplar_transform is not None:
            self.store_ext = self._full_ext(n)                       # host [rows][2]: valid (h, w) of every stored frame
        self.store_t = torch.zeros((n, self.n_outputs), dtype=torch.float32, device=self.device)     # mem_class_y rows
        self._store_lab = torch.zeros((n,), dtype=torch.int64, device=self.device)      # (the assemble kernel copies a label per row)
        if rows and rows["_rows_x"].shape[0]:
            idx = torch.tensor(self.stored_rows(), dtype=torch.int64, device=self.device)
            self.store_x[idx] = rows["_rows_x"]
            self.store_t[idx] = rows["_rows_t"]
            if self.exemplar_transform is not None:
                self.store_ext[idx.cpu()] = rows["_rows_ext"]

    # ------------------------------------------------------------------ features / training output
    def features(self, x):
        """get_feature (:203-207) of any number of rows: the un-masked input of the first Linear layer, [n][n_feat]."""
        out = []
        for s in range(0, x.shape[0], self.engine.max_batch):
            xb = x[s:s + self.engine.max_batch].contiguous()
            self.engine.forward(xb)
            out.append(self.engine.layer_input(self.fc_first, xb.shape[0]).clone())
        return torch.cat(out)

    def forward_training(self, x, t):
        """:188-201: the head's output of any number of rows, -10e10 outside the task's slice (dropout as the net's mode
        says, fresh masks per pass)."""
        out = []
        for s in range(0, x.shape[0], self.engine.max_batch):
            xb = x[s:s + self.engine.max_batch].contiguous()
            self._dropout(xb.shape[0])
            out.append(self.engine.forward(xb))
        return self._mask_slice(torch.cat(out), t)

    # ------------------------------------------------------------------ memory (:314-479)
    def _truncate(self, new_count):
        """Every stored class keeps its first new_count entries; the class blocks are compacted in place."""
        self.class_len = [min(n, new_count) for n in self.class_len]
        stores = (self.store_x, self.store_t) + (() if self.exemplar_transform is None else (self.store_ext,))
        compact_blocks(stores, self.exemplar_count, new_count, self.class_len)
        self.exemplar_count = new_count

    def herd(self, feats, ranges, weights, ks):
        """ops.icarl_herd over feats [n_rows][F] (device fp32): ranges = [(row_begin, row_end)] per class, weights the
        per-row mean weights (device fp32 [n_rows]), ks the picks per class.  Returns the device int32 ranking (classes
        back to back) and the offsets of the classes in it.  No synchronisation."""
        return ops.icarl_herd(feats, weights, ranges, ks, flat=True)

    def manage_memory(self, t, args):
        """:314-479 for task t: truncate the stored classes to K/m entries, rank K_c = min(K/m, class size) exemplars of
        every class of the task (features once, one herding launch), store them with their distillation targets."""
        if self.engine.bns:
            raise NotImplementedError("icarl: herding ranks features computed once, which a net with BatchNorm in `features` "
                                      "does not have (they depend on the batch)")
        if t != self.old_task:
            self.init_new_task(t)
        count = int(self.n_total_memories / self.cum_nc_per_task[t])          # K/m
        assert count > 0, "Each class should get at least 1 exemplar"
        o1, o2 = compute_offsets(t, self.cum_nc_per_task)
        if len(self.class_len) != o1:
            raise RuntimeError("icarl: manage_memory(%d) needs the classes of the earlier tasks stored (%d of %d)"
                               % (t, len(self.class_len), o1))
        self._truncate(count)
        train = args.task_imgfolders["train"]
        if self.exemplar_transform is not None:
            return self._manage_memory_frames(t, train, count, int(args.batch_size))
        if getattr(train, "transform", None) is not None:
            raise NotImplementedError("icarl: herding ranks the stored images of the task; an augmented split (%r) stores frames "
                                      "larger than the net's input" % (train.transform,))
        if isinstance(train, ByteTaskDataset):
            train = train.decoded()                                             # a byte split: herding reads the frames it means
        x, y = train.x, train.y
        order = torch.sort(y, stable=True)[1]                                   # classes back to back, dataset order inside
        sizes = torch.bincount(y, minlength=o2 - o1).cpu().tolist()
        if len(sizes) != o2 - o1 or min(sizes) <= 0:
            raise ValueError("icarl: every class of the task needs at least one training image, got sizes %s" % sizes)
        F = self.engine.layer_input(self.fc_first, 1).shape[1]
        if F > HERD_MAX_FEATS:
            raise NotImplementedError("icarl: %d features > %d of the herding kernel" % (F, HERD_MAX_FEATS))
        was_training = self.net.training
        self.net.train(False)
        self._dropout(1)
        feats = self.features(x).index_select(0, order)     # features in dataset order; only the small matrix is put in class order
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        ranges = [(int(bounds[c]), int(bounds[c + 1])) for c in range(o2 - o1)]
        ks = [min(count, n) for n in sizes]
        w = torch.from_numpy(np.concatenate([mean_weights(n, int(args.batch_size)) for n in sizes])).to(self.device)
        ranking, offs = self.herd(feats, ranges, w, ks)
        base = torch.from_numpy(np.repeat(bounds[:-1], ks)).to(self.device)
        rows = base + ranking[:int(offs[-1])].long()                            # rows in class order, class after class
        dst = torch.from_numpy(np.concatenate([(o1 + c) * count + np.arange(ks[c]) for c in range(o2 - o1)])).to(self.device)
        exemplars = x.index_select(0, order.index_select(0, rows))
        self.store_x[dst] = exemplars
        self.store_t[dst] = self.forward_training(exemplars, t)                 # :476-479, eval mode
        self.class_len.extend(ks)
        self.last_ranking = (ranking, offs)
        self.net.train(was_training)
        self._means = {}

    # ------------------------------------------------------------------ frame mode: views of stored frames
    def view_params(self, t, kind, ext):
        """Host int32 [n][params_width]: one draw of the train transform per frame of valid sizes ext [n][2], in that order, from
        a private CPU generator seeded view_seed_of(self.view_seed, t, kind).  No global generator is touched."""
        return self.draw_exemplar_params(ext, view_seed_of(self.view_seed, t, kind))

    def _gather_view(self, table, idx, params):
        """The loaders' gather of this wrapper's spec and store kind: crops [len(idx)][C][th][tw] of the frames in `table`."""
        spec = self.exemplar_transform
        if isinstance(spec, RandomPadCropFlip):
            pad = (self.geometry, spec.padding_mode, spec.padding, self.fill)
            if self.frame_norm is None:
                return ops.gather_tasks_pad_crop_flip(table, *pad, idx, params)[0]
            return ops.gather_tasks_pad_crop_flip_u8(table, *pad, self.lut, idx, params)[0]
        resized = isinstance(spec, RandomResizedCropFlip)
        if self.frame_norm is None:
            gather = ops.gather_tasks_resized_crop_flip if resized else ops.gather_tasks_crop_flip
            return gather(table, self.geometry, idx, params)[0]
        gather = ops.gather_tasks_resized_crop_flip_u8 if resized else ops.gather_tasks_crop_flip_u8
        return gather(table, self.geometry, self.lut, idx, params)[0]

    def _assemble_step(self, x, y, B, gather_dev, params_dev):
        """The step-assembly launch of this wrapper's spec and store kind: x_mix, y_mix and t_mix[B:B + E) in one launch."""
        spec = self.exemplar_transform
        args = (x, y, B, self.store_x, gather_dev, params_dev, self.store_t, self.x_mix, self.y_mix, self.t_mix)
        if isinstance(spec, RandomPadCropFlip):
            pad = (self.geometry, spec.padding_mode, spec.padding, self.fill)
            if self.frame_norm is None:
                ops.icarl_assemble_pad_crop_flip(*pad, *args)
            else:
                ops.icarl_assemble_pad_crop_flip_u8(*pad, self.lut, *args)
            return
        resized = isinstance(spec, RandomResizedCropFlip)
        if self.frame_norm is None:
            (ops.icarl_assemble_resized_crop_flip if resized else ops.icarl_assemble_crop_flip)(self.geometry, *args)
        else:
            (ops.icarl_assemble_resized_crop_flip_u8 if resized else ops.icarl_assemble_crop_flip_u8)(self.geometry, self.lut, *args)

    def _manage_memory_frames(self, t, train, count, batch_size):
        """manage_memory on an augmented split (the store is truncated already).  The reference runs the class loader once
        per pick (:394-451): with a random train transform every pick sees new crops of every image.  Here ONE draw per
        training image, the herding view (view_params(t, VIEW_HERD, the split's extents), dataset order), stands for all
        passes: features once on those crops, mean weights, ranking and K_c as in crop mode; the winners' FRAMES and extents
        go to the store, their targets are forward_training of their herding-view crops (:476-479)."""
        spec = _transform_of(train)
        if spec is None:
            raise ValueError("icarl: a frame-mode wrapper herds the frames of an augmented train split; this one carries no transform")
        if _spec_key(spec) != _spec_key(self.exemplar_transform):
            raise ValueError("icarl: the train split carries %r, the wrapper replays %r" % (spec, self.exemplar_transform))
        byte = isinstance(train, ByteTaskDataset)
        ext = spec.extents if spec.extents is not None else self._full_ext(len(train))
        self._check_source(BatchSource(train.x, None, None, ext, (train.mean, train.std) if byte else None))
        o1, o2 = compute_offsets(t, self.cum_nc_per_task)
        y, n = train.y, len(train)
        order = torch.sort(y, stable=True)[1]
        sizes = torch.bincount(y, minlength=o2 - o1).cpu().tolist()
        if len(sizes) != o2 - o1 or min(sizes) <= 0:
            raise ValueError("icarl: every class of the task needs at least one training image, got sizes %s" % sizes)
        F = self.engine.layer_input(self.fc_first, 1).shape[1]
        if F > HERD_MAX_FEATS:
            raise NotImplementedError("icarl: %d features > %d of the herding kernel" % (F, HERD_MAX_FEATS))
        herd_params = self.view_params(t, VIEW_HERD, ext)
        params_dev = herd_params.to(self.device)
        table = ops.task_table([train.x], [train.y], [n], [0], self.device)
        was_training = self.net.training
        self.net.train(False)
        self._dropout(1)
        step, feats = self.engine.max_batch, []
        for s in range(0, n, step):                                             # the chunks of features()
            idx = torch.arange(s, min(n, s + step), dtype=torch.int64, device=self.device)
            feats.append(self.features(self._gather_view(table, idx, params_dev[s:s + step].contiguous())))
        feats = torch.cat(feats).index_select(0, order)
        bounds = np.concatenate([[0], np.cumsum(sizes)])
        ranges = [(int(bounds[c]), int(bounds[c + 1])) for c in range(o2 - o1)]
        ks = [min(count, m) for m in sizes]
        w = torch.from_numpy(np.concatenate([mean_weights(m, batch_size) for m in sizes])).to(self.device)
        ranking, offs = self.herd(feats, ranges, w, ks)
        base = torch.from_numpy(np.repeat(bounds[:-1], ks)).to(self.device)
        rows = base + ranking[:int(offs[-1])].long()
        dst = torch.from_numpy(np.concatenate([(o1 + c) * count + np.arange(ks[c]) for c in range(o2 - o1)]))
        win = order.index_select(0, rows)                                       # sample numbers of the winners, class after class
        self.store_x[dst.to(self.device)] = train.x.index_select(0, win)
        self.store_ext[dst] = ext.index_select(0, win.cpu())
        crops = torch.cat([self._gather_view(table, win[s:s + step].contiguous(), params_dev.index_select(0, win[s:s + step]))
                           for s in range(0, win.shape[0], step)])
        self.store_t[dst.to(self.device)] = self.forward_training(crops, t)     # :476-479, eval mode
        self.class_len.extend(ks)
        self.last_ranking = (ranking, offs)
        self.last_herd_params = herd_params
        self.net.train(was_training)
        self._means = {}

    def exemplar_params(self, gather, seeds):
        """Frame mode: host int32 [len(gather)][params_width], one fresh draw per gathered store row in gather order over the
        rows' own extents (RehearsalNet.exemplar_params's rule: the generator is seeded with the base seed the plan's last
        exemplar loader drew anyway, so the global generators are consumed exactly as in crop mode)."""
        if not gather:
            return torch.zeros((0, self.params_width), dtype=torch.int32)
        return self.draw_exemplar_params(self.store_ext[torch.tensor(gather, dtype=torch.int64)], seeds[-1])

    # ------------------------------------------------------------------ the steps
    def observe_FT(self, x, t, y, source=None):
        """:209-223: CE on the task's slice of the current batch only, SGD step.  source: the batch's BatchSource in frame mode
        (checked only: iCaRL copies nothing from the batch), None in crop mode."""
        self._check_source(source)
        self.net.train(True)
        self._means = {}
        self.stats.zero_()
        self._dropout(x.shape[0])
        loss, _ = self.engine.loss_step(x, y, "ce_mean", True, self.stats, class_slice=compute_offsets(t, self.cum_nc_per_task))
        self.opt.step()
        return loss, self.stats[1]

    def plan(self, t, seeds=None):
        return exemplar_draws(t, self.n_append, self.class_len, self.exemplar_count, self.nc_per_task, self.cum_nc_per_task,
                              self.total_batch_size, seeds)

    def observe(self, x, t, y, source=None):
        """:229-246 -> update_representation (:482-598).  Returns device (loss, hits on the current batch) and the batch_stats
        dictionary the shared training loop reads (no projections here).  source: as observe_FT.  Frame mode: every gathered
        exemplar gets a fresh draw (exemplar_params), and ONE clhip_icarl_assemble_* launch fills x_mix, y_mix and t_mix[B:N)."""
        self._check_source(source)
        frames = self.exemplar_transform is not None
        self.net.train(True)
        self._means = {}
        if t != self.old_task:
            self.init_new_task(t)
        B = int(y.shape[0])
        seeds = []
        _, plan = self.plan(t, seeds)
        scales = segment_scales([len(chunks) for _, chunks in plan], float(self.reg))
        segs = [(0, B) + self._slice(t) + (1.0, 0)]
        gather = []
        for (past, chunks), sc in zip(plan, scales):
            for ch in chunks:
                segs.append((B + len(gather), B + len(gather) + len(ch)) + self._slice(past) + (sc, 1))
                gather.extend(c * self.exemplar_count + e for c, e in ch)
        E, N, n = len(gather), B + len(gather), len(segs)
        if N > self.batch_size:
            raise RuntimeError("icarl: step of %d rows > engine batch %d" % (N, self.batch_size))
        # two tables in the one upload: the mixed batch's rows, then each segment alone from row 0 (the segmented path)
        local = [(0, sg[1] - sg[0]) + sg[2:] for sg in segs]
        self.last_gather = list(gather)
        if frames:
            self.last_exemplar_params = self.exemplar_params(gather, seeds)
            gather_dev, tabs, params_dev = self._upload(gather, ops.loss_segment_rows(segs + local), self.last_exemplar_params)
            self._assemble_step(x, y, B, gather_dev if E else None, params_dev if E else None)
        else:
            gather_dev, tabs = self._upload(gather, ops.loss_segment_rows(segs + local))
            L = _lib.lib()
            check(L.clhip_rehearsal_assemble(
                x.data_ptr(), y.data_ptr(), B, int(np.prod(self.in_shape)), self.store_x.data_ptr(), self._store_lab.data_ptr(),
                self.store_x.shape[0], 0, 0, gather_dev.data_ptr() if E else None, E, self.x_mix.data_ptr(), self.y_mix.data_ptr(),
                _stream()), "clhip_rehearsal_assemble")
            if E:                      # the stored distillation rows of the same exemplars -> t_mix[B:N)
                check(L.clhip_rehearsal_assemble(
                    None, None, 0, self.n_outputs, self.store_t.data_ptr(), self._store_lab.data_ptr(), self.store_t.shape[0], 0, 0,
                    gather_dev.data_ptr(), E, self.t_mix[B:].data_ptr(), self._scratch_lab.data_ptr(), _stream()),
                    "clhip_rehearsal_assemble")
        xm, ym = self.x_mix[:N], self.y_mix[:N]
        masks = self._dropout(N)
        self.stats.zero_()
        if self._fused(N, n):
            loss = self.engine.loss_step_segments(xm, ym, tabs[:6 * n], n, self.stats, targets=self.t_mix, T=T_DISTILL)[0].clone()
        else:
            loss = self._segmented(xm, ym, segs, tabs[6 * n:], masks)
        self.opt.step()
        return loss, self.stats[1], {"projected_grads": []}

    def _segmented(self, xm, ym, segs, segs_local, masks):
        """The reference's order: the current batch, then every chunk (tasks ascending); one forward / loss / backward per
        segment (its rows of the step's masks, its own one-row segment table)."""
        loss = torch.zeros(1, dtype=torch.float32, device=self.device)

        def one_pass(g):
            r0, r1 = segs[g][:2]
            for li, m in masks.items():
                self.engine.set_dropout(li, m[r0:r1])
            logits = self.engine.forward(xm[r0:r1])
            _, dz = ops.loss_segments(logits, ym[r0:r1], self.t_mix[r0:r1], segs_local[6 * g:], 1, T_DISTILL,
                                      self.stats if g == 0 else None, loss=loss)
            self.engine.backward(xm[r0:r1], dz)
            return loss, 1.0
        return self._accumulate(range(len(segs)), one_pass)

    # ------------------------------------------------------------------ evaluation
    def class_means(self, t, batch_size):
        """[nc_t][n_feat] means of the stored exemplars of task t: per class the mean of batch means (:160-167) over the
        exemplars in STORED order in batches of batch_size; None while the task's first class has no exemplars.
        Frame mode: the stored frames are cropped under ONE draw of the train transform, the class-mean view
        (view_params(t, VIEW_MEANS, the rows' extents), stored order), by the assembly launch with B = 0 in chunks of the
        engine's batch; the reference redraws per evaluated batch (forward's docstring)."""
        key = (t, int(batch_size))
        if key not in self._means:
            o1, o2 = compute_offsets(t, self.cum_nc_per_task)
            if o1 >= len(self.class_len):
                self._means[key] = None
            else:
                if o2 > len(self.class_len):
                    raise RuntimeError("icarl: task %d is stored in part only" % t)
                rows = [c * self.exemplar_count + e for c in range(o1, o2) for e in range(self.class_len[c])]
                if self.exemplar_transform is None:
                    feats = self.features(self.store_x.index_select(0, torch.tensor(rows, dtype=torch.int64, device=self.device)))
                else:
                    feats = self._view_features(t, rows)
                means, lo = [], 0
                for c in range(o1, o2):
                    n = self.class_len[c]
                    w = torch.from_numpy(mean_weights(n, int(batch_size))).to(self.device).double()
                    means.append((feats[lo:lo + n].double() * w[:, None]).sum(0).float())
                    lo += n
                self._means[key] = torch.stack(means).contiguous()
        return self._means[key]

    def _view_features(self, t, rows):
        """Features of the class-mean view of the store rows `rows` (class_means, frame mode)."""
        params = self.view_params(t, VIEW_MEANS, self.store_ext[torch.tensor(rows, dtype=torch.int64)])
        gather_dev = torch.tensor(rows, dtype=torch.int32).to(self.device)
        params_dev = params.to(self.device)
        step, out = self.engine.max_batch, []
        for s in range(0, len(rows), step):
            n = min(step, len(rows) - s)
            self._assemble_step(None, None, 0, gather_dev[s:s + n], params_dev[s:s + n].contiguous())
            out.append(self.features(self.x_mix[:n]))
        return torch.cat(out)

    def __call__(self, x, t, args=None, train_mode=False, **kw):
        return self.forward(x, t, args, train_mode)

    def forward(self, x, t, args=None, train_mode=False):
        """:130-186 (eval): the 1-of-C code of the nearest class mean among the classes of task t (zeros, 1 at the class);
        for a task without exemplars -10e10 everywhere and 1/nc inside its slice.

        The class means are computed once per (model, task, evaluation batch size) and cached, not once per batch.  One
        difference from the reference: its exemplar loader is shuffled, this one takes the stored order; the mean of batch
        means depends on the order only when a class holds more exemplars than one batch and the last batch is short.
        Frame mode, a second one: the reference's exemplar loader carries the train transform, so it recomputes the means
        from freshly cropped exemplars for every evaluated batch (:160-167); here they come from one draw per (model, task,
        batch size), the class-mean view (class_means), so an evaluation is reproducible."""
        if train_mode:
            return self.forward_training(x, t)
        self._eval_dropout(1)
        bs = int(getattr(args, "batch_size", self.batch_size)) if args is not None else self.batch_size
        means = self.class_means(t, bs)
        o1, o2 = compute_offsets(t, self.cum_nc_per_task)
        N = x.shape[0]
        out = torch.empty((N, self.n_outputs), dtype=torch.float32, device=self.device)
        feats = self.features(x) if means is not None else None
        check(_lib.lib().clhip_icarl_nme(feats.data_ptr() if feats is not None else None,
                                         means.data_ptr() if means is not None else None, N,
                                         feats.shape[1] if feats is not None else 0, o2 - o1, o1, self.n_outputs, out.data_ptr(),
                                         _stream()), "clhip_icarl_nme")
        return out
