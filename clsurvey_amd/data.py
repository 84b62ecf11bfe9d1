"""Device-resident task data.

The reference trains on pickled ImageFolder datasets that re-decode 8000 JPEGs per epoch through
8 DataLoader workers (EWC/main_EWC.py:28-31, data/imgfolder.py:86-128).  The framework uses the
raw, un-augmented sets (framework/main.py:197-202), so a whole Tiny-ImageNet task is a static
393 MB tensor: here it lives in HBM once and batches are gathered on device.

`DeviceLoader` reproduces the batch composition of torch's DataLoader(shuffle=True) bit for bit
for the same global torch RNG state (it consumes the global generator exactly like
_BaseDataLoaderIter.__init__ + RandomSampler.__iter__ do), so accuracy traces can be compared with
the reference run under the same seed (utilities/utils.py:52-58).

A split may carry a `RandomCropFlip` spec (the `train` split of a RecogSeq task, the `rnd_transform` file of iNaturalist):
its stored frames stay static in HBM and the loaders crop and mirror them inside the gather that assembles each batch
(clhip_gather_tasks_crop_flip), a fresh draw per sample per epoch.  A `RandomResizedCropFlip` spec (the `train` split of the
cropped Tiny-ImageNet variant) is served the same way by the gather that resamples (clhip_gather_tasks_resized_crop_flip), and a
`RandomPadCropFlip` spec (torchvision's RandomCrop(size, padding, fill, padding_mode) + flip, the CIFAR-style rule for frames already
at the net's input size) by the gather that pads (clhip_gather_tasks_pad_crop_flip): the stored frames carry no margin.

A split may also hold its frames as the decoded uint8 images (`ByteTaskDataset`): ToTensor -> Normalize, the last step of every
Compose of the reference, then happens inside the same gathers through a 256-entry table per channel (the ..._u8 entries of
include/clhip.h), and the batches are bitwise those of the fp32 split `.decoded()` returns.
"""
import math

import torch
from torch.utils.data import Dataset


class RandomCropFlip(object):
    """RandomCrop(size) + RandomHorizontalFlip(p) of stored frames (data/recogseq_dataprep.py:56-57,
    data/inaturalist_dataprep.py:240-241) as a picklable spec: it holds no image tensor and does nothing by itself, the loaders
    apply it.  size = (th, tw).  extents: optional host int tensor [n][2], the valid (h, w) of every stored frame — Resize(256)
    fixes only the shorter side, so real frames differ in size and are stored top-left anchored in a common Hs x Ws frame;
    None: every frame is full."""

    def __init__(self, size, p=0.5, extents=None):
        th, tw = (int(v) for v in size)
        if th < 1 or tw < 1 or not 0.0 <= float(p) <= 1.0:
            raise ValueError("RandomCropFlip: size >= 1 and 0 <= p <= 1, got %s, %s" % (size, p))
        self.size = (th, tw)
        self.p = float(p)
        self.extents = None if extents is None else torch.as_tensor(extents, dtype=torch.int64).cpu().reshape(-1, 2)

    def __repr__(self):
        return "RandomCropFlip(size=%s, p=%s%s)" % (self.size, self.p, "" if self.extents is None else ", extents=[%d][2]" % len(self.extents))


RESIZE_MAX_RATIO = 8          # CLHIP_RESIZE_MAX_RATIO (include/clhip.h): the largest extent / size the resampling gather takes


class RandomResizedCropFlip(object):
    """RandomResizedCrop(size, scale, ratio) + RandomHorizontalFlip(p) of stored frames (data/tinyimgnet_dataprep.py:105-122,
    the cropped Tiny-ImageNet variant; the standard ImageNet training augmentation) as a picklable spec like RandomCropFlip —
    a class of its own, not a subclass: code that asks isinstance(t, RandomCropFlip) never takes one for the other.
    size = (th, tw) of the output, scale the range of the window's share of the image area, ratio the range of its aspect
    w / h, extents as in RandomCropFlip."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p=0.5, extents=None):
        th, tw = (int(v) for v in size)
        scale, ratio = tuple(float(v) for v in scale), tuple(float(v) for v in ratio)
        if th < 1 or tw < 1 or not 0.0 <= float(p) <= 1.0:
            raise ValueError("RandomResizedCropFlip: size >= 1 and 0 <= p <= 1, got %s, %s" % (size, p))
        if len(scale) != 2 or len(ratio) != 2 or not 0.0 < scale[0] <= scale[1] or not 0.0 < ratio[0] <= ratio[1]:
            raise ValueError("RandomResizedCropFlip: 0 < scale[0] <= scale[1] and 0 < ratio[0] <= ratio[1], got %s, %s" % (scale, ratio))
        self.size = (th, tw)
        self.scale = scale
        self.ratio = ratio
        self.p = float(p)
        self.extents = None if extents is None else torch.as_tensor(extents, dtype=torch.int64).cpu().reshape(-1, 2)

    def __repr__(self):
        return "RandomResizedCropFlip(size=%s, scale=%s, ratio=%s, p=%s%s)" % (
            self.size, self.scale, self.ratio, self.p, "" if self.extents is None else ", extents=[%d][2]" % len(self.extents))


PAD_MODES = ("constant", "edge", "reflect", "symmetric")      # torchvision's padding_mode; the position is the gathers' `mode`
PAD_MAX = 32767               # CLHIP_PAD_MAX (include/clhip.h): the largest pad the padded gathers take


class RandomPadCropFlip(object):
    """torchvision's RandomCrop(size, padding, fill, padding_mode) + RandomHorizontalFlip(p) of stored frames (pad, crop, then
    hflip; RandomCrop(32, padding=4) + flip is the standard augmentation of the CIFAR-style split benchmarks) as a picklable spec
    like RandomCropFlip — a class of its own, not a subclass: code that asks isinstance(t, RandomCropFlip) never takes one for
    the other.  size = (th, tw) of the output.  padding: an int, (left/right, top/bottom) or (left, top, right, bottom), kept
    as (pl, pt, pr, pb); it goes around each sample's valid extent, not around the common storage frame.  padding_mode: one of
    PAD_MODES.  fill (read by `constant` only): one value per channel IN THE DOMAIN OF THE STORED FRAMES, a scalar or a
    C-sequence: floats (the normalised value) on a TensorTaskDataset, ints in 0..255 on a ByteTaskDataset, where byte v of
    channel c means lut()[c][v] (torchvision pads the decoded image before ToTensor -> Normalize).  extents as in RandomCropFlip.
    pad_if_needed is not built."""

    def __init__(self, size, padding, fill=0, padding_mode="constant", p=0.5, extents=None):
        th, tw = (int(v) for v in size)
        if th < 1 or tw < 1 or not 0.0 <= float(p) <= 1.0:
            raise ValueError("RandomPadCropFlip: size >= 1 and 0 <= p <= 1, got %s, %s" % (size, p))
        if isinstance(padding, (list, tuple)):
            pads = tuple(padding)
        elif isinstance(padding, bool) or not isinstance(padding, int):
            raise ValueError("RandomPadCropFlip: padding is an int or a sequence of 2 or 4 ints, got %r" % (padding,))
        else:
            pads = (padding,)
        if len(pads) not in (1, 2, 4) or any(isinstance(v, bool) or not isinstance(v, int) for v in pads):
            raise ValueError("RandomPadCropFlip: padding is an int or a sequence of 2 or 4 ints, got %r" % (padding,))
        pads = pads * 4 if len(pads) == 1 else pads * 2 if len(pads) == 2 else pads
        if min(pads) < 0 or max(pads) > PAD_MAX:
            raise ValueError("RandomPadCropFlip: pads in 0..%d, got %r" % (PAD_MAX, padding))
        if padding_mode not in PAD_MODES:
            raise ValueError("RandomPadCropFlip: padding_mode is one of %s, got %r" % (PAD_MODES, padding_mode))
        if isinstance(fill, (list, tuple)):
            fill = tuple(fill)
            vals = fill
            if not vals:
                raise ValueError("RandomPadCropFlip: fill is a number or one number per channel, got %r" % (fill,))
        else:
            vals = (fill,)
        if any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in vals):
            raise ValueError("RandomPadCropFlip: fill is a number or one number per channel, got %r" % (fill,))
        self.size = (th, tw)
        self.padding = pads
        self.fill = fill
        self.padding_mode = padding_mode
        self.p = float(p)
        self.extents = None if extents is None else torch.as_tensor(extents, dtype=torch.int64).cpu().reshape(-1, 2)

    def fill_values(self, C, byte=False):
        """The C fill values, checked: one per channel, and on byte frames ints in 0..255."""
        vals = self.fill if isinstance(self.fill, tuple) else (self.fill,) * int(C)
        if len(vals) != int(C):
            raise ValueError("RandomPadCropFlip: %d fill values for %d channels" % (len(vals), C))
        if byte and any(not isinstance(v, int) or not 0 <= v <= 255 for v in vals):
            raise ValueError("RandomPadCropFlip: the fill of byte frames is ints in 0..255, got %r" % (self.fill,))
        return vals

    def __repr__(self):
        return "RandomPadCropFlip(size=%s, padding=%s, fill=%s, padding_mode=%r, p=%s%s)" % (
            self.size, self.padding, self.fill, self.padding_mode, self.p,
            "" if self.extents is None else ", extents=[%d][2]" % len(self.extents))


def draw_pad_crop_flip(n, spec, frame_hw, generator, order=None):
    """int32 [n][5] of (top, left, flip, h, w), one row per position of an epoch: the window's corner uniform over the padded
    image of the sample served there (RandomCrop.get_params after the pad), in the sample's UNPADDED coordinates: with
    (pl, pt, pr, pb) = spec.padding, i = min(floor(u0 (h + pt + pb - th + 1)), h + pt + pb - th) and top = i - pt in
    [-pt, h + pb - th]; left likewise from u1 in [-pl, w + pr - tw]; flip = u2 < spec.p.  (h, w) is frame_hw, or with
    spec.extents the extent of the sample (extents[order[k]], as in draw_crop_flip).  One torch.rand((n, 3), float64) call: with
    all pads 0 the first three columns are bitwise draw_crop_flip's from the same generator state.
    Raises if a padded extent is smaller than spec.size, an extent is empty or exceeds the frame, or the pads exceed what the
    mode takes for the smallest extent (reflect: extent - 1, symmetric: extent, as torch.nn.functional.pad)."""
    th, tw = spec.size
    pl, pt, pr, pb = spec.padding
    Hs, Ws = (int(v) for v in frame_hw)
    n = int(n)
    if spec.extents is None:
        h = torch.full((n,), Hs, dtype=torch.int64)
        w = torch.full((n,), Ws, dtype=torch.int64)
    else:
        ext = spec.extents if order is None else spec.extents.index_select(0, torch.as_tensor(order, dtype=torch.int64))
        if ext.shape[0] != n:
            raise ValueError("draw_pad_crop_flip: %d extents for %d positions" % (ext.shape[0], n))
        h, w = ext[:, 0], ext[:, 1]
    if n:
        hmin, wmin = int(h.min()), int(w.min())
        if hmin < 1 or wmin < 1:
            raise ValueError("draw_pad_crop_flip: an empty extent")
        if hmin + pt + pb < th or wmin + pl + pr < tw:
            raise ValueError("draw_pad_crop_flip: a frame of %d x %d padded by %s is smaller than the crop %d x %d"
                             % (hmin, wmin, spec.padding, th, tw))
        if int(h.max()) > Hs or int(w.max()) > Ws:
            raise ValueError("draw_pad_crop_flip: an extent exceeds the stored frame %d x %d" % (Hs, Ws))
        slack = {"reflect": 1, "symmetric": 0}.get(spec.padding_mode)
        if slack is not None and (max(pt, pb) > hmin - slack or max(pl, pr) > wmin - slack):
            raise ValueError("draw_pad_crop_flip: padding_mode %r takes pads up to the extent%s, got %s for a frame of %d x %d"
                             % (spec.padding_mode, " - 1" if slack else "", spec.padding, hmin, wmin))
    u = torch.rand((n, 3), generator=generator, dtype=torch.float64)
    top = torch.minimum((u[:, 0] * (h + (pt + pb - th + 1))).floor().long(), h + (pt + pb - th)) - pt
    left = torch.minimum((u[:, 1] * (w + (pl + pr - tw + 1))).floor().long(), w + (pl + pr - tw)) - pl
    flip = (u[:, 2] < spec.p).long()
    return torch.stack([top, left, flip, h, w], 1).to(torch.int32).contiguous()


def draw_crop_flip(n, spec, frame_hw, generator, order=None):
    """int32 [n][3] of (top, left, flip), one row per position of an epoch: top uniform on [0, h - th] and left on [0, w - tw],
    both inclusive (RandomCrop.get_params), flip = 1 with probability spec.p (RandomHorizontalFlip: rand < p).  (h, w) is
    frame_hw, or with spec.extents the extent of the sample served at that position: extents[order[k]] (order None: sample k).
    One torch.rand call for the whole epoch.  Raises if an extent is smaller than spec.size or larger than the frame.

    The reference draws these inside 4-8 DataLoader worker processes seeded base_seed + worker id, and which worker gets which
    sample depends on scheduling: that stream cannot be reproduced by a batch loader.  The draws here have the same
    distribution and are a deterministic function of the generator's seed."""
    th, tw = spec.size
    Hs, Ws = (int(v) for v in frame_hw)
    n = int(n)
    if spec.extents is None:
        h = torch.full((n,), Hs, dtype=torch.int64)
        w = torch.full((n,), Ws, dtype=torch.int64)
    else:
        ext = spec.extents if order is None else spec.extents.index_select(0, torch.as_tensor(order, dtype=torch.int64))
        if ext.shape[0] != n:
            raise ValueError("draw_crop_flip: %d extents for %d positions" % (ext.shape[0], n))
        h, w = ext[:, 0], ext[:, 1]
    if n and (int(h.min()) < th or int(w.min()) < tw):
        raise ValueError("draw_crop_flip: a frame of %d x %d is smaller than the crop %d x %d"
                         % (int(h.min()), int(w.min()), th, tw))
    if n and (int(h.max()) > Hs or int(w.max()) > Ws):
        raise ValueError("draw_crop_flip: an extent exceeds the stored frame %d x %d" % (Hs, Ws))
    u = torch.rand((n, 3), generator=generator, dtype=torch.float64)
    top = torch.minimum((u[:, 0] * (h - th + 1)).floor().long(), h - th)
    left = torch.minimum((u[:, 1] * (w - tw + 1)).floor().long(), w - tw)
    flip = (u[:, 2] < spec.p).long()
    return torch.stack([top, left, flip], 1).to(torch.int32).contiguous()


SPECS = (RandomCropFlip, RandomResizedCropFlip, RandomPadCropFlip)


RESIZED_TRIES = 10            # RandomResizedCrop.get_params: tries before the central fallback window


def draw_resized_crop_flip(n, spec, frame_hw, generator, order=None):
    """int32 [n][5] of (top, left, h, w, flip), one row per position of an epoch: RandomResizedCrop.get_params on the extent
    (H, W) of the sample served there (frame_hw, or extents[order[k]] as in draw_crop_flip).  Up to 10 tries of
    area = H W U(scale), aspect = exp(U(log ratio[0], log ratio[1])), w = round(sqrt(area aspect)), h = round(sqrt(area /
    aspect)) (Python's round: half to even), the first with 0 < w <= W and 0 < h <= H wins and gets top uniform on [0, H - h],
    left uniform on [0, W - w].  Otherwise the central window clamped to the ratio range: w = W, h = round(W / ratio[0]) when
    W / H < ratio[0]; h = H, w = round(H ratio[1]) when W / H > ratio[1]; else the whole extent; top = (H - h) // 2,
    left = (W - w) // 2 (a side that rounds to 0 or past the extent is clamped into [1, extent]).  flip = 1 with probability
    spec.p.  ALL uniforms of the epoch come from one torch.rand call of 2 x 10 + 3 columns per row (areas, aspects, top, left,
    flip), whether a row uses them or not: the table is a function of the generator's seed and of `order` alone.
    Raises if an extent exceeds the frame or RESIZE_MAX_RATIO times the size (the window could be one the gather rejects).

    torchvision draws these numbers one by one from the global generator inside the DataLoader workers (see draw_crop_flip):
    same distribution, a deterministic function of the seed here."""
    th, tw = spec.size
    Hs, Ws = (int(v) for v in frame_hw)
    n = int(n)
    if spec.extents is None:
        H = torch.full((n,), Hs, dtype=torch.int64)
        W = torch.full((n,), Ws, dtype=torch.int64)
    else:
        ext = spec.extents if order is None else spec.extents.index_select(0, torch.as_tensor(order, dtype=torch.int64))
        if ext.shape[0] != n:
            raise ValueError("draw_resized_crop_flip: %d extents for %d positions" % (ext.shape[0], n))
        H, W = ext[:, 0], ext[:, 1]
    if n and (int(H.min()) < 1 or int(W.min()) < 1):
        raise ValueError("draw_resized_crop_flip: an empty extent")
    if n and (int(H.max()) > Hs or int(W.max()) > Ws):
        raise ValueError("draw_resized_crop_flip: an extent exceeds the stored frame %d x %d" % (Hs, Ws))
    if n and (int(H.max()) > RESIZE_MAX_RATIO * th or int(W.max()) > RESIZE_MAX_RATIO * tw):
        raise ValueError("draw_resized_crop_flip: an extent of %d x %d is more than %d times the output %d x %d"
                         % (int(H.max()), int(W.max()), RESIZE_MAX_RATIO, th, tw))
    K = RESIZED_TRIES
    u = torch.rand((n, 2 * K + 3), generator=generator, dtype=torch.float64)
    Hf, Wf = H.double()[:, None], W.double()[:, None]
    area = Hf * Wf * (spec.scale[0] + u[:, :K] * (spec.scale[1] - spec.scale[0]))
    l0, l1 = math.log(spec.ratio[0]), math.log(spec.ratio[1])
    aspect = torch.exp(l0 + u[:, K:2 * K] * (l1 - l0))
    w = torch.round(torch.sqrt(area * aspect))                    # (torch.round is half to even, as Python's)
    h = torch.round(torch.sqrt(area / aspect))
    ok = (w > 0) & (w <= Wf) & (h > 0) & (h <= Hf)
    first = ok.int().argmax(1, keepdim=True) if n else torch.zeros((0, 1), dtype=torch.int64)   # (the first maximum)
    found = ok.any(1)
    w, h = w.gather(1, first)[:, 0].long(), h.gather(1, first)[:, 0].long()
    top = torch.minimum((u[:, 2 * K] * (H - h + 1).double()).floor().long(), H - h)
    left = torch.minimum((u[:, 2 * K + 1] * (W - w + 1).double()).floor().long(), W - w)
    # the fallback of the rows no try served
    in_ratio = W.double() / H.double()
    fw = torch.where(in_ratio > spec.ratio[1], torch.round(H.double() * spec.ratio[1]).long(), W)
    fh = torch.where(in_ratio < spec.ratio[0], torch.round(W.double() / spec.ratio[0]).long(), H)
    fw, fh = torch.minimum(fw.clamp(min=1), W), torch.minimum(fh.clamp(min=1), H)
    w, h = torch.where(found, w, fw), torch.where(found, h, fh)
    top, left = torch.where(found, top, (H - fh) // 2), torch.where(found, left, (W - fw) // 2)
    flip = (u[:, 2 * K + 2] < spec.p).long()
    return torch.stack([top, left, h, w, flip], 1).to(torch.int32).contiguous()


def _spec_key(t):
    """What two specs must share to be served as one (the extents are per task)."""
    return (type(t), t.size, t.p, getattr(t, "scale", None), getattr(t, "ratio", None),
            getattr(t, "padding", None), getattr(t, "padding_mode", None), getattr(t, "fill", None))


def _respec(t, extents=None):
    """`t` with other extents."""
    if isinstance(t, RandomResizedCropFlip):
        return RandomResizedCropFlip(t.size, t.scale, t.ratio, t.p, extents)
    if isinstance(t, RandomPadCropFlip):
        return RandomPadCropFlip(t.size, t.padding, t.fill, t.padding_mode, t.p, extents)
    return RandomCropFlip(t.size, t.p, extents)


def _transform_of(dataset):
    """The RandomCropFlip, RandomResizedCropFlip or RandomPadCropFlip a dataset carries, else None (any other `transform`
    attribute is the dataset's own business)."""
    t = getattr(dataset, "transform", None)
    return t if isinstance(t, SPECS) else None


def norm_lut(mean, std):
    """CPU fp32 [C][256], the meaning of a byte per channel: ToTensor (uint8 -> float, / 255) then Normalize (- mean, / std),
    op for op as torchvision does them, of all 256 byte values."""
    return (torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)[None, :] - mean[:, None]) / std[:, None]


def merged_norm(dsets):
    """(mean, std) of several tasks served as one dataset when they hold byte frames, None when they hold floats.  All are
    ByteTaskDatasets with equal mean and std, or none is: anything else is a ValueError (one table decodes a batch)."""
    dsets = list(dsets)
    byte = [isinstance(d, ByteTaskDataset) for d in dsets]
    if not any(byte):
        return None
    if not all(byte):
        raise ValueError("tasks served as one dataset all hold byte frames or all hold floats: %s" % [type(d).__name__ for d in dsets])
    mean, std = dsets[0].mean, dsets[0].std
    if any(not (torch.equal(d.mean, mean) and torch.equal(d.std, std)) for d in dsets):
        raise ValueError("byte tasks served as one dataset share mean and std: %s" % [(d.mean.tolist(), d.std.tolist()) for d in dsets])
    return mean, std


def merged_transform(dsets):
    """One spec for several tasks served as one dataset: all carry a spec of one class with equal parameters (extents
    concatenated in task order, a task without them counts as full frames), or none carries a transform.  The tasks also
    agree on how their frames are stored (merged_norm)."""
    merged_norm(dsets)
    ts = [_transform_of(d) for d in dsets]
    if all(t is None for t in ts):
        return None
    if any(t is None for t in ts) or any(_spec_key(t) != _spec_key(ts[0]) for t in ts):
        raise ValueError("tasks served as one dataset carry equal RandomCropFlip size and p (a RandomPadCropFlip: and equal "
                         "padding, mode and fill), or none: %s" % ts)
    if all(t.extents is None for t in ts):
        return _respec(ts[0])
    ext = [t.extents if t.extents is not None else torch.tensor(tuple(d.x.shape[-2:])).repeat(len(d), 1) for t, d in zip(ts, dsets)]
    return _respec(ts[0], torch.cat(ext))


class TensorTaskDataset(Dataset):
    """One split of one task. `classes` mirrors ImageFolder_Subset.classes (data/imgfolder.py).  `transform`: None, a
    RandomCropFlip or a RandomResizedCropFlip.  It is applied by the loaders only (DeviceLoader, MultiTaskLoader): `dataset[i]` and `.x` stay the stored
    frames, so code that reads them directly sees what it is handed."""

    transform = None          # class-level default: task files pickled before the attribute existed still load

    def __init__(self, x, y, classes, transform=None):
        assert x.shape[0] == y.shape[0]
        self.x = x.contiguous().float()
        self.y = y.contiguous().long()
        self.classes = list(classes)
        self._set_transform(transform)

    def _set_transform(self, transform):
        if transform is not None:
            if not isinstance(transform, SPECS):
                raise TypeError("TensorTaskDataset: transform is None or a RandomCropFlip")
            if isinstance(transform, RandomPadCropFlip):
                transform.fill_values(self.x.shape[1], byte=self.x.dtype == torch.uint8)
            if transform.extents is not None and len(transform.extents) != len(self):
                raise ValueError("TensorTaskDataset: %d extents for %d frames" % (len(transform.extents), len(self)))
            self.transform = transform

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.y[i]


class ByteTaskDataset(TensorTaskDataset):
    """A split whose frames stay the decoded uint8 images [n][C][H][W], with the per-channel `mean` and `std` of the
    reference's Normalize.  It MEANS the fp32 split of lut()[c][x]: the loaders decode inside their gathers (a quarter of the
    bytes in HBM, in the task cache and on the source side of every gather) and serve, bitwise, what they serve for
    `decoded()`.  `.x` and `dataset[i]` stay bytes: code that reads frames directly goes through `decoded()`."""

    def __init__(self, x_u8, y, classes, mean, std, transform=None):
        if not torch.is_tensor(x_u8) or x_u8.dtype != torch.uint8:
            raise TypeError("ByteTaskDataset: frames are a uint8 tensor, got %s" % (getattr(x_u8, "dtype", type(x_u8)),))
        if x_u8.dim() != 4:
            raise ValueError("ByteTaskDataset: frames [n, C, H, W], got %s" % (tuple(x_u8.shape),))
        assert x_u8.shape[0] == y.shape[0]
        mean = torch.as_tensor(mean, dtype=torch.float32).detach().cpu().reshape(-1).clone()
        std = torch.as_tensor(std, dtype=torch.float32).detach().cpu().reshape(-1).clone()
        C = int(x_u8.shape[1])
        if mean.numel() != C or std.numel() != C:
            raise ValueError("ByteTaskDataset: %d channels, %d means, %d stds" % (C, mean.numel(), std.numel()))
        if not bool(torch.isfinite(mean).all()) or not bool(torch.isfinite(std).all()) or not bool((std > 0).all()):
            raise ValueError("ByteTaskDataset: mean finite, std finite and > 0, got %s, %s" % (mean.tolist(), std.tolist()))
        self.x = x_u8.contiguous()
        self.y = y.contiguous().long()
        self.classes = list(classes)
        self.mean, self.std = mean, std
        self._set_transform(transform)

    def lut(self):
        """CPU fp32 [C][256]: the table the loaders decode through (norm_lut)."""
        return norm_lut(self.mean, self.std)

    def decoded(self):
        """The equivalent TensorTaskDataset (same labels, classes and transform), frames looked up in lut()."""
        lut = self.lut().to(self.x.device)
        x = torch.empty(self.x.shape, dtype=torch.float32, device=self.x.device)
        for c in range(self.x.shape[1]):
            plane = self.x[:, c]
            x[:, c] = lut[c].index_select(0, plane.reshape(-1).int()).view(plane.shape)
        t = self.transform
        if isinstance(t, RandomPadCropFlip):           # its fill is bytes here: the decoded split's is what they mean
            t = RandomPadCropFlip(t.size, t.padding, self.decoded_fill(t), t.padding_mode, t.p, t.extents)
        return TensorTaskDataset(x, self.y, self.classes, transform=t)

    def decoded_fill(self, spec):
        """The fill of a RandomPadCropFlip on these frames in the decoded domain: lut()[c][fill byte of c], one float a channel."""
        lut = self.lut()
        return tuple(float(lut[c, v]) for c, v in enumerate(spec.fill_values(self.x.shape[1], byte=True)))


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
        if isinstance(dset, ByteTaskDataset):
            out[split] = ByteTaskDataset(x.to(device), y.to(device), dset.classes, dset.mean, dset.std, transform=_transform_of(dset))
        else:
            out[split] = TensorTaskDataset(x.to(device), y.to(device), getattr(dset, "classes", []), transform=_transform_of(dset))
        nbytes += _split_bytes(out[split])
    limit = float(os.environ.get("CLHIP_DATA_CACHE_GB", "64")) * 2 ** 30
    while _TASK_CACHE and _TASK_CACHE_BYTES[0] + nbytes > limit:
        old = next(iter(_TASK_CACHE))
        _TASK_CACHE_BYTES[0] -= sum(_split_bytes(d) for d in _TASK_CACHE.pop(old).values())
    if nbytes <= limit:
        _TASK_CACHE[key] = out
        _TASK_CACHE_BYTES[0] += nbytes
    return out


def _split_bytes(d):
    """What a cached split holds in HBM (fp32 frames: 4 bytes an element, byte frames: 1)."""
    return d.x.numel() * d.x.element_size() + d.y.numel() * 8


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
    torch.utils.data.DataLoader(dataset, batch_size, shuffle, drop_last=False).

    A dataset that carries a RandomCropFlip is served augmented: the stored frames stay under `.frames`, `.x` is a zero-row
    tensor of the OUTPUT row shape (C, th, tw) (what callers size their engine from), and every epoch draws one (top, left, flip)
    per position in serving order from a private CPU generator seeded with the base seed `order()` draws anyway (the
    _BaseDataLoaderIter draw), shuffle or not.  The global generator is consumed exactly as without a transform, so an augmented
    loader serves the same sample order as a plain one from the same RNG state.  The table is uploaded once per epoch and
    sliced per batch: one clhip_gather_tasks_crop_flip launch per batch, no host read.  While iterating, `last_idx` (device
    int64) and `last_idx_host` hold the sample numbers of the batch just served: with `frames` they are what an exemplar wrapper
    in frame mode stores instead of the crop (methods/exemplar.py: the counterpart of the reference's `paths`).  Difference from
    the reference: its draws happen in DataLoader worker processes (see draw_crop_flip).
    A RandomResizedCropFlip is served by the same steps: the table holds (top, left, h, w, flip) rows from
    draw_resized_crop_flip and the launch is clhip_gather_tasks_resized_crop_flip.
    A ByteTaskDataset is ALWAYS served through a gather, with or without a transform (the ..._u8 entry of the gather the fp32
    split would take; clhip_gather_tasks_u8 with idx = arange when there is neither a transform nor a shuffle): `.x`, `.frames`,
    `last_idx` and `last_idx_host` behave as in augmented mode, `.transform` stays what the dataset carries.  The table of the
    byte values is uploaded once per loader.  Batches, labels and the consumption of the generators are those of the loader
    over `dataset.decoded()`.
    A RandomPadCropFlip is served by the same steps too: (top, left, flip, h, w) rows from draw_pad_crop_flip, the launch
    clhip_gather_tasks_pad_crop_flip[_u8]; a crop larger than the stored frame is legal when the padded image holds it.  The
    fill vector (on byte frames lut[c][fill byte of c]) is uploaded once per loader."""

    transform = None
    _resized = False
    _padded = False
    _fill = None              # device float32 [C] of a RandomPadCropFlip, output domain
    _norm = None              # (mean, std) of byte frames
    _lut = None
    base_seed = None
    last_idx = last_idx_host = None

    def __init__(self, dataset, batch_size, shuffle, device="cuda"):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.device = torch.device(device)
        x, y = _extract(dataset)
        self.x = x.to(self.device)
        self.y = y.to(self.device)
        self.n = self.x.shape[0]
        transform = _transform_of(dataset)
        self._norm = merged_norm([dataset])
        if transform is not None:
            self._augment(transform, [self.x], [self.y], [self.n], [0])
        elif self._norm is not None:
            self._serve_bytes([self.x], [self.y], [self.n], [0])

    def _serve_bytes(self, xs, ys, cum_rows, label_shifts):
        """Serve the byte frames xs (one tensor per task) without a transform: decoded by the plain gather."""
        if any(tuple(v.shape[1:]) != tuple(xs[0].shape[1:]) for v in xs):
            raise ValueError("byte tasks of one sequence share the frame shape")
        self.frames = xs
        self.row_shape = tuple(int(v) for v in xs[0].shape[1:])
        self.x = torch.empty((0,) + self.row_shape, dtype=torch.float32, device=xs[0].device)
        self._sources = (xs, ys, list(cum_rows), list(label_shifts))
        self._table = None

    def _augment(self, transform, xs, ys, cum_rows, label_shifts):
        """Serve `transform` of the frames xs (one tensor per task)."""
        if xs[0].dim() != 4 or any(tuple(v.shape[1:]) != tuple(xs[0].shape[1:]) for v in xs):
            raise ValueError("%s needs frames [n, C, Hs, Ws] of one shape" % type(transform).__name__)
        C, Hs, Ws = (int(v) for v in xs[0].shape[1:])
        th, tw = transform.size
        if (th > Hs or tw > Ws) and isinstance(transform, RandomCropFlip):      # (a resized window may be enlarged, a padded image larger)
            raise ValueError("%s: crop %d x %d of frames %d x %d" % (type(transform).__name__, th, tw, Hs, Ws))
        if transform.extents is not None and len(transform.extents) != self.n:
            raise ValueError("%s: %d extents for %d frames" % (type(transform).__name__, len(transform.extents), self.n))
        self.transform = transform
        self._resized = isinstance(transform, RandomResizedCropFlip)
        self._padded = isinstance(transform, RandomPadCropFlip)
        if self._padded:
            transform.fill_values(C, byte=self._norm is not None)
        self.frames = xs
        self.geometry = (C, Hs, Ws, th, tw)
        self.x = torch.empty((0, C, th, tw), dtype=torch.float32, device=xs[0].device)    # (row shape only: what engine_for reads; no memory)
        self._sources = (xs, ys, list(cum_rows), list(label_shifts))
        self._table = None                          # device table, built at the first epoch (order() alone needs no device)

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def order(self):
        # _BaseDataLoaderIter.__init__ draws the worker base seed first ...
        self.base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        if not self.shuffle:
            return None
        # ... then RandomSampler.__iter__ seeds a private generator from the global one
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(self.n, generator=g)

    def epoch_params(self, perm):
        """Host int32 table of the epoch whose order() returned `perm` (None: dataset order): [n][3] rows of draw_crop_flip,
        [n][5] rows of draw_resized_crop_flip, or [n][5] rows of draw_pad_crop_flip."""
        g = torch.Generator()
        g.manual_seed(self.base_seed)
        draw = draw_resized_crop_flip if self._resized else draw_pad_crop_flip if self._padded else draw_crop_flip
        return draw(self.n, self.transform, self.geometry[1:3], g, order=perm)

    def _augmented(self, perm):
        from . import ops
        if self._table is None:
            self._table = ops.task_table(*self._sources, self.device)
            if self._norm is not None:
                self._lut = norm_lut(*self._norm).to(self.device)
            if self._padded:
                fill = self.transform.fill_values(self.geometry[0], byte=self._norm is not None)
                if self._norm is not None:          # a byte means what the table says
                    lut = norm_lut(*self._norm)
                    fill = [lut[c, v] for c, v in enumerate(fill)]
                self._fill = torch.tensor([float(v) for v in fill], dtype=torch.float32).to(self.device)
        params = self.epoch_params(perm).to(self.device) if self.transform is not None else None
        idx_host = torch.arange(self.n) if perm is None else perm
        idx = idx_host.to(self.device)
        pad = (self.transform.padding_mode, self.transform.padding, self._fill) if self._padded else ()
        if self._norm is None:
            gather, lut = (ops.gather_tasks_resized_crop_flip if self._resized else ops.gather_tasks_pad_crop_flip if self._padded
                           else ops.gather_tasks_crop_flip), ()
        else:
            gather, lut = (ops.gather_tasks_resized_crop_flip_u8 if self._resized else ops.gather_tasks_pad_crop_flip_u8
                           if self._padded else ops.gather_tasks_crop_flip_u8), (self._lut,)
        for s in range(0, self.n, self.batch_size):
            self.last_idx, self.last_idx_host = idx[s:s + self.batch_size], idx_host[s:s + self.batch_size]
            if params is None:                      # byte frames without a transform: whole rows
                x, y = ops.gather_tasks_u8(self._table, self.row_shape[0], math.prod(self.row_shape[1:]), self._lut, self.last_idx)
                yield x.view((x.shape[0],) + self.row_shape), y
            else:
                yield gather(self._table, self.geometry, *pad, *lut, self.last_idx, params[s:s + self.batch_size])

    def __iter__(self):
        perm = self.order()
        if self.transform is not None or self._norm is not None:
            yield from self._augmented(perm)
            return
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
        merged_norm(self.datasets)                    # all byte frames with one mean / std, or all floats
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
    task the cache already holds) is never built.  Tasks that carry a RandomCropFlip, a RandomResizedCropFlip or a RandomPadCropFlip (all of one class and
    equal parameters, or none) are served augmented as DeviceLoader describes, the crop and flip done in the same gather.
    Tasks that hold byte frames (all of them, with equal mean and std) are decoded in the same gather; no merged copy either."""

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
        transform = merged_transform(dataset.datasets)
        self._norm = merged_norm(dataset.datasets)
        if transform is not None:
            self._augment(transform, xs, ys, dataset.cumulative_sizes, dataset.label_shifts)
            return
        if self._norm is not None:
            self._serve_bytes(xs, ys, dataset.cumulative_sizes, dataset.label_shifts)
            return
        self.table = ops.task_table(xs, ys, dataset.cumulative_sizes, dataset.label_shifts, self.device)

    def __iter__(self):
        from . import ops
        perm = self.order()
        if self.transform is not None or self._norm is not None:
            if perm is not None and self.n:
                self.dataset.locate(perm[[int(perm.argmin()), int(perm.argmax())]])               # host check, before any launch
            yield from self._augmented(perm)
            return
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
