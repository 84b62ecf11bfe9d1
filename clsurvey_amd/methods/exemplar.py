"""What the exemplar methods (GEM, the rehearsal baselines R-PM / R-FM, iCaRL) share on the HIP path: a wrapper around a
net and its NetEngine that pickles like the reference's nn.Module, evaluates on a task's slice of the shared head, and runs
a training step over [current batch | exemplar chunks] either as ONE fused pass (clhip_net_loss_step_loss_segments) or,
for a plan with BatchNorm or a step over the loss kernel's limits, segment by segment with clhip_axpy accumulation.

A method derives from ExemplarNet and one of the two dropout policies and keeps what is its own: the store layout, the
host draws, the memory management and the composition of its step.

Frame mode (GEM, R-PM / R-FM): the reference's memories hold image PATHS, and every replay rebuilds the exemplar loader with
the current task's train transform (gem.py:233-234, baseline_rehearsal_partial_mem.py:215-216, common.py:57-72), so an
exemplar is cropped and mirrored afresh at every draw.  A wrapper built with a RandomCropFlip spec does the same: its store
holds the loader's FRAMES (copied by sample number: BatchSource, the counterpart of the reference's `paths`), `store_ext`-style
host tables hold each stored frame's valid (h, w), and the crop happens when the exemplars are replayed.

Byte store (frame mode with frame_norm = (mean, std)): the loader holds uint8 frames (data.ByteTaskDataset) and the store holds
their bytes; a stored byte v of channel c means norm_lut(mean, std)[c][v], decoded where the exemplars are replayed
(clhip_rehearsal_assemble_crop_flip_u8, GEM: the ..._u8 crop gather of its memory loader).  One table decodes a store, so every
batch source carries the store's mean and std.

Resized replay (frame mode with a RandomResizedCropFlip spec, the cropped Tiny-ImageNet rule): the replayed exemplar is a fresh
RandomResizedCrop window of its stored frame, drawn over the frame's own extent and resampled inside the assembly launch
(clhip_rehearsal_assemble_resized_crop_flip[_u8], the block body of the loaders' resizing gather); the draws are rows of
(top, left, h, w, flip).  Store, ring update and extents are those of frame mode.

Padded replay (frame mode with a RandomPadCropFlip spec, the CIFAR-style rule RandomCrop(size, padding) + flip): the store holds
the UNPADDED frames and the replayed exemplar is a fresh window of its padded frame, drawn over the frame's own extent and padded
inside the assembly launch (clhip_rehearsal_assemble_pad_crop_flip[_u8], the block body of the loaders' padded gather); the draws
are rows of (top, left, flip, h, w).  A frame may be smaller than the crop.  The wrapper keeps the spec's fill as a transient
device vector; on a byte store the spec's fill is bytes and the vector holds what they decode to.

iCaRL in frame mode (icarl.py): the same store of frames, extents and replay draws, but its exemplars are chosen by herding, not
copied out of the batches, and each carries a distillation row.  Two things need ONE fixed image of a randomly transformed
frame: the ranking (the herding view, one draw per training image at manage_memory) and the class means of the nearest-mean
classifier (the class-mean view, one draw per stored exemplar).  Both come from a private CPU generator seeded by
icarl.view_seed_of(view_seed, task, kind), a function of those three alone.  The step is assembled by clhip_icarl_assemble_*: the
exemplar windows and their stored distillation rows in one launch.
"""
import collections

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from ..data import (RandomCropFlip, RandomPadCropFlip, RandomResizedCropFlip, _respec, draw_crop_flip, draw_pad_crop_flip,
                    draw_resized_crop_flip, norm_lut)
from ..net import NetEngine

FUSED_MAX_ROWS, FUSED_MAX_SEGS = ops.LOSS_MAX_ROWS, ops.LOSS_MAX_SEGS        # the fused loss's limits (include/clhip.h)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def compute_offsets(task_idx, cum_nc_per_task):
    """rehearsal/model/common.py:106-118."""
    o1 = 0 if task_idx == 0 else int(cum_nc_per_task[task_idx - 1])
    return o1, int(cum_nc_per_task[task_idx])


# Where a batch of an augmented loader came from: the loader's frame tensor, the sample numbers it just gathered (device and
# host), the valid (h, w) of the loader's frames (host int64 [n][2], None: every frame is full) and, for uint8 frames, their
# (mean, std) (CPU fp32 [C] each; None: the frames are floats).
BatchSource = collections.namedtuple("BatchSource", ["frames", "idx", "idx_host", "extents", "norm"], defaults=(None,))


def batch_source(loader):
    """The BatchSource of the batch `loader` served last; None for a loader without a transform."""
    spec = getattr(loader, "transform", None)
    if spec is None:
        return None
    if len(loader.frames) != 1:
        raise ValueError("exemplar frames are copied out of ONE frame tensor (a DeviceLoader over one task)")
    return BatchSource(loader.frames[0], loader.last_idx, loader.last_idx_host, spec.extents, getattr(loader, "_norm", None))


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

    _TRANSIENT = ("engine", "A", "stats", "opt", "x_mix", "y_mix", "_acc", "lut", "fill")
    _TRANSIENT_POLICY = ()          # the dropout policy's state
    _TRANSIENT_EXTRA = ()           # the subclass's own device state
    _HOST_ROWS = ("_rows_ext",)     # rows of _rows_state() that stay on the host

    # class-level defaults: a wrapper pickled before frame mode existed loads in crop mode
    exemplar_transform = None       # RandomCropFlip(size, p), RandomResizedCropFlip(size, scale, ratio, p) or RandomPadCropFlip(
                                    # size, padding, fill, padding_mode, p) of the replayed exemplars, or None: the store holds crops
    frame_shape = None              # (C, Hs, Ws) of the stored frames
    frame_norm = None               # (mean, std), CPU fp32 [C] each: the frames are stored as uint8 and mean norm_lut(mean, std)
    lut = None                      # device fp32 [C][256] of a byte store (transient: rebuilt by _bind)
    fill = None                     # device fp32 [C] of a RandomPadCropFlip, output domain (transient: rebuilt by _bind)

    def _init_frames(self, exemplar_transform, frame_shape, frame_norm=None):
        """Frame mode on (a spec and the frame shape) or off (both None).  in_shape stays the crop shape.  frame_norm = (mean,
        std): the frames are stored as bytes."""
        if exemplar_transform is None:
            if frame_shape is not None and tuple(frame_shape) != tuple(self.in_shape):
                raise ValueError("exemplar wrapper: a frame shape needs an exemplar_transform")
            if frame_norm is not None:
                raise ValueError("exemplar wrapper: a byte store holds frames (frame_norm needs an exemplar_transform)")
            return
        if not isinstance(exemplar_transform, (RandomCropFlip, RandomResizedCropFlip, RandomPadCropFlip)) or frame_shape is None:
            raise TypeError("exemplar wrapper: exemplar_transform is a RandomCropFlip and comes with the frame shape (C, Hs, Ws) "
                            "(or a RandomResizedCropFlip: resized replay; or a RandomPadCropFlip: padded replay)")
        C, Hs, Ws = (int(v) for v in frame_shape)
        pl, pt, pr, pb = getattr(exemplar_transform, "padding", (0, 0, 0, 0))      # (the PADDED frame holds the crop)
        if (C,) + exemplar_transform.size != tuple(self.in_shape) or Hs + pt + pb < self.in_shape[1] or Ws + pl + pr < self.in_shape[2]:
            raise ValueError("exemplar wrapper: frames %s, crop %s, net input %s" % (tuple(frame_shape), exemplar_transform.size,
                                                                                 self.in_shape))
        if isinstance(exemplar_transform, RandomPadCropFlip):
            slack = {"reflect": 1, "symmetric": 0}.get(exemplar_transform.padding_mode)
            if slack is not None and (max(pt, pb) > Hs - slack or max(pl, pr) > Ws - slack):
                raise ValueError("exemplar wrapper: padding_mode %r takes pads up to the extent%s, got %s for frames of %d x %d"
                                 % (exemplar_transform.padding_mode, " - 1" if slack else "", exemplar_transform.padding, Hs, Ws))
            exemplar_transform.fill_values(C, byte=frame_norm is not None)          # (one per channel; bytes on a byte store)
        self.exemplar_transform = _respec(exemplar_transform)                                       # (the extents are a task's)
        self.frame_shape = (C, Hs, Ws)
        if frame_norm is not None:
            mean, std = (torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1).clone() for v in frame_norm)
            if mean.numel() != C or std.numel() != C:
                raise ValueError("exemplar wrapper: %d channels, %d means, %d stds" % (C, mean.numel(), std.numel()))
            self.frame_norm = (mean, std)

    @property
    def store_dtype(self):
        """Element type of the exemplar store."""
        return torch.float32 if self.frame_norm is None else torch.uint8

    @property
    def params_width(self):
        """Columns of an exemplar's draw: (top, left, flip), (top, left, h, w, flip) of a resized spec, or (top, left, flip, h, w)
        of a padded one."""
        return 5 if isinstance(self.exemplar_transform, (RandomResizedCropFlip, RandomPadCropFlip)) else 3

    def _assemble(self, *args):
        """The frame-mode assembly launch of this wrapper's spec and store kind (ops.rehearsal_assemble_crop_flip's arguments
        after the geometry)."""
        spec = self.exemplar_transform
        if isinstance(spec, RandomPadCropFlip):
            pad = (self.geometry, spec.padding_mode, spec.padding, self.fill)
            if self.frame_norm is None:
                ops.rehearsal_assemble_pad_crop_flip(*pad, *args)
            else:
                ops.rehearsal_assemble_pad_crop_flip_u8(*pad, self.lut, *args)
            return
        resized = isinstance(spec, RandomResizedCropFlip)
        if self.frame_norm is None:
            (ops.rehearsal_assemble_resized_crop_flip if resized else ops.rehearsal_assemble_crop_flip)(self.geometry, *args)
        else:
            (ops.rehearsal_assemble_resized_crop_flip_u8 if resized else ops.rehearsal_assemble_crop_flip_u8)(
                self.geometry, self.lut, *args)

    @property
    def store_shape(self):
        """Row shape of the exemplar store."""
        return self.in_shape if self.exemplar_transform is None else self.frame_shape

    @property
    def geometry(self):
        return self.frame_shape + self.exemplar_transform.size

    def _full_ext(self, rows):
        """Host int64 [rows][2]: every frame full."""
        return torch.tensor(self.frame_shape[1:], dtype=torch.int64).repeat(rows, 1)

    def _check_source(self, source):
        """A frame-mode wrapper takes batches with their BatchSource, a crop-mode one without."""
        if self.exemplar_transform is None:
            if source is not None:
                raise ValueError("exemplar wrapper in crop mode handed a batch with its frames (build it with exemplar_transform)")
            return
        if source is None:
            raise ValueError("exemplar wrapper in frame mode handed a plain batch: it stores frames by sample number "
                             "(pass batch_source(loader))")
        if tuple(source.frames.shape[1:]) != self.frame_shape:
            raise ValueError("exemplar wrapper: frames %s, store %s" % (tuple(source.frames.shape[1:]), self.frame_shape))
        if source.frames.dtype != self.store_dtype or (source.norm is None) != (self.frame_norm is None):
            raise ValueError("exemplar wrapper: %s frames %s mean / std for a %s store (a byte store takes byte frames with their "
                             "mean and std, an fp32 store float frames)"
                             % (source.frames.dtype, "without" if source.norm is None else "with", self.store_dtype))
        if self.frame_norm is not None and not all(torch.equal(torch.as_tensor(a, dtype=torch.float32).cpu().reshape(-1), b)
                                                   for a, b in zip(source.norm, self.frame_norm)):
            raise ValueError("exemplar wrapper: one table decodes a byte store; the batch's mean / std %s differ from the store's %s"
                             % ([torch.as_tensor(v).tolist() for v in source.norm], [v.tolist() for v in self.frame_norm]))

    def _source_ext(self, source, n):
        """Host int64 [n][2]: the valid (h, w) of the first n samples of the batch."""
        if source.extents is None:
            return self._full_ext(n)
        return source.extents.index_select(0, source.idx_host[:n])

    def draw_exemplar_params(self, ext, seed):
        """Host int32 [n][3] of (top, left, flip) for exemplars whose frames have the valid sizes ext [n][2], in that order, from
        a private CPU generator: the global one is not touched (DeviceLoader's rule for its epoch table).  A resized spec:
        [n][5] of (top, left, h, w, flip), RandomResizedCrop's windows over the same extents.  A padded spec: [n][5] of (top,
        left, flip, h, w), draw_pad_crop_flip's corners over the padded extents."""
        g = torch.Generator()
        g.manual_seed(seed)
        spec = _respec(self.exemplar_transform, ext)
        draw = (draw_resized_crop_flip if isinstance(spec, RandomResizedCropFlip) else
                draw_pad_crop_flip if isinstance(spec, RandomPadCropFlip) else draw_crop_flip)
        return draw(ext.shape[0], spec, self.frame_shape[1:], g)

    def _bind(self, mix=True):
        """Engine and work buffers; mix: the [current batch | exemplar chunks] rows of a step."""
        rows = max(self.batch_size, 1)
        self.engine = NetEngine(self.net, rows, self.in_shape, self.device)
        self.engine.auto_dropout = False        # the masks are the wrapper's own (its dropout policy), not the engine's
        self.A = self.engine.arena
        self.stats = torch.zeros(2, dtype=torch.float64, device=self.device)
        lut = None if self.frame_norm is None else norm_lut(*self.frame_norm)
        self.lut = None if lut is None else lut.to(self.device)
        self.fill = None
        if isinstance(self.exemplar_transform, RandomPadCropFlip):
            fill = self.exemplar_transform.fill_values(self.frame_shape[0], byte=lut is not None)
            if lut is not None:                 # a byte means what the table says (ByteTaskDataset.decoded_fill)
                fill = [lut[c, v] for c, v in enumerate(fill)]
            self.fill = torch.tensor([float(v) for v in fill], dtype=torch.float32).to(self.device)
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
        self._load_rows({k: v if k in self._HOST_ROWS else v.to(self.device) for k, v in rows.items()})
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
    def _upload(self, gather, rows, params=None):
        """Gather rows (int32), rows of int32 columns (clhip_loss_segment tables: ops.loss_segment_rows) and, in frame mode, the
        exemplars' draws (int32 [len(gather)][params_width]) in ONE pinned host buffer, one non-blocking copy.  Returns
        the device parts, the second one flat; the third one only when params is given."""
        n, m = len(gather), rows.size
        width = 0 if params is None else self.params_width
        pinned = torch.empty(n + m + width * n, dtype=torch.int32, pin_memory=True)
        host = pinned.numpy()
        host[:n] = gather
        host[n:n + m] = rows.reshape(-1)
        if params is not None:
            host[n + m:] = params.numpy().reshape(-1)
        dev = pinned.to(self.device, non_blocking=True)     # the caching host allocator keeps `pinned` until the copy ran
        if params is None:
            return dev[:n], dev[n:]
        return dev[:n], dev[n:n + m], dev[n + m:].view(n, width)

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
