"""Task-sequence dataset objects with the interface of src/data/dataset.py CustomDataset
(name, argname, test_results_dir, train_exp_results_dir, task_count, classes_per_task, input_size,
get_task_dataset_path(task_name, rnd_transform), get_taskname(i)).

There is no Tiny-ImageNet in the container (no network), so `SyntheticTinyImagenet` writes tensor
tasks of the same shape (10 tasks x 20 classes, 8000/2000/1000 images of 3x64x64,
data/tinyimgnet_dataprep.py:69-151) — class-conditional Gaussian prototypes + noise so accuracies
and forgetting are non-trivial — as pickled {'train','val','test'} dicts, the same wire format the
reference's framework passes between its layers."""
import json
import os
from collections import OrderedDict

import torch

from ..data import PAD_MODES, ByteTaskDataset, RandomCropFlip, RandomPadCropFlip, RandomResizedCropFlip, TensorTaskDataset, synthetic_task


class SyntheticTaskSequence(object):
    def __init__(self, root, task_count=10, classes_per_task=20, sizes=(8000, 2000, 1000), hw=64, seed=7, noise=1.0,
                 name="synthetic_tiny_imagenet", kind="protos", blobs=None, rnd_margin=0, rnd_always=False, rnd_resized=0,
                 u8_frames=False, rnd_pad=0, pad_mode="constant"):
        """rnd_margin = m > 0: images are generated at (hw + m)^2; task_N.pth.tar holds their centre hw^2 crops (the Resize(256) /
        CenterCrop(224) of get_transforms(), data/inaturalist_dataprep.py:256-277) and task_N_rndtrans.pth.tar (named after
        data/dataset.py:108) the same images with the full frames + RandomCropFlip((hw, hw)) as `train` split.  rnd_always: the
        RecogSeq rule, get_task_dataset_path ignores its rnd_transform argument (data/dataset.py:458-466).  rnd_margin = 0:
        every byte written and every path returned is what it was before the option existed.
        rnd_resized = m > 0 (instead of rnd_margin): the cropped Tiny-ImageNet variant (data/tinyimgnet_dataprep.py:105-122,
        crop=True).  The same two files of the same images; the `train` split of task_N_rndtrans.pth.tar holds the full
        (hw + m)^2 frames with RandomResizedCropFlip((hw, hw)) (RandomResizedCrop(56) of 64^2 images), every other split the
        centre hw^2 crops (Resize(64) of a 64-pixel image is the identity, then CenterCrop(56)).  0: as if the option did
        not exist.
        u8_frames: the same generated images, quantised as clamp(round(x * 48 + 128), 0, 255), are stored as ByteTaskDatasets
        with mean = 128 / 255 and std = 48 / 255 on every channel (what a pipeline that keeps the decoded images hands over), in
        both files of a task and with either margin option.  False: as if the option did not exist.
        rnd_pad = m > 0 (instead of rnd_margin / rnd_resized): the CIFAR-style rule, RandomCrop(hw, padding=m) + flip of images
        ALREADY at the net's input size.  Images are generated at hw^2, no margin; both files of a task hold the same images and
        the `train` split of task_N_rndtrans.pth.tar carries RandomPadCropFlip((hw, hw), padding=m, padding_mode=pad_mode) with
        fill 0.0, or with u8_frames byte 128, which decodes to exactly 0.0 under the mean and std above.  0: as if the option
        did not exist."""
        self.name = name
        self.argname = name
        self.test_results_dir = name
        self.train_exp_results_dir = name
        self.task_count = task_count
        self.input_size = (hw, hw)
        self.classes_per_task = OrderedDict((self.get_taskname(i), [str(c) for c in range(classes_per_task)])
                                            for i in range(1, task_count + 1))
        self.root = root
        self.sizes = sizes
        self.hw = hw
        self.seed = seed
        self.noise = noise
        self.kind = kind
        self.blobs = blobs
        self.n_classes = classes_per_task
        self.rnd_margin = int(rnd_margin)
        self.rnd_always = bool(rnd_always)
        self.rnd_resized = int(rnd_resized)
        self.u8_frames = bool(u8_frames)
        self.rnd_pad = int(rnd_pad)
        self.pad_mode = str(pad_mode)
        if self.rnd_margin < 0 or self.rnd_resized < 0 or self.rnd_pad < 0:
            raise ValueError("SyntheticTaskSequence: rnd_margin >= 0, rnd_resized >= 0 and rnd_pad >= 0")
        if bool(self.rnd_margin) + bool(self.rnd_resized) + bool(self.rnd_pad) > 1:
            raise ValueError("SyntheticTaskSequence: one of rnd_margin, rnd_resized and rnd_pad, not several")
        if self.pad_mode not in PAD_MODES:
            raise ValueError("SyntheticTaskSequence: pad_mode is one of %s, got %r" % (PAD_MODES, pad_mode))

    def get_taskname(self, task_index):
        return str(task_index)

    def spec(self, task_name, rnd_transform=False):
        """Everything the bytes of a task file depend on (without a margin: the same keys as ever, existing caches stay hits)."""
        out = {"sizes": [int(v) for v in self.sizes], "classes": int(self.n_classes), "hw": int(self.hw),
               "seed": int(self.seed) * 1000 + int(task_name), "noise": float(self.noise), "kind": str(self.kind),
               "blobs": None if self.blobs is None else {k: float(v) for k, v in sorted(dict(self.blobs).items())}}
        if self.rnd_margin:
            out["rnd_margin"] = self.rnd_margin
        if self.rnd_resized:
            out["rnd_resized"] = self.rnd_resized
        if self.rnd_pad:
            out["rnd_pad"] = self.rnd_pad
            out["pad_mode"] = self.pad_mode
        if (self.rnd_margin or self.rnd_resized or self.rnd_pad) and rnd_transform:
            out["rnd_transform"] = True
        if self.u8_frames:
            out["u8_frames"] = True
        return out

    def _split(self, x, y, classes, transform=None):
        """One split of a file: floats, or with u8_frames the quantised bytes."""
        if not self.u8_frames:
            return TensorTaskDataset(x, y, classes, transform=transform)
        C = x.shape[1]
        return ByteTaskDataset((x * 48 + 128).round().clamp(0, 255).to(torch.uint8), y, classes, [128.0 / 255] * C, [48.0 / 255] * C,
                               transform=transform)

    def _make(self, task_name, rnd_transform):
        """The {'train', 'val', 'test'} dict of one file."""
        want = self.spec(task_name)
        m = self.rnd_margin or self.rnd_resized
        d = synthetic_task(self.sizes[0], self.sizes[1], self.sizes[2], self.n_classes, self.hw + m,
                           seed=want["seed"], noise=self.noise, kind=self.kind, blobs=self.blobs)
        if self.rnd_pad:                           # no margin: the padded crop jitters frames of the output size
            spec = RandomPadCropFlip((self.hw, self.hw), padding=self.rnd_pad, fill=128 if self.u8_frames else 0.0,
                                     padding_mode=self.pad_mode) if rnd_transform else None
            return {s: self._split(v.x, v.y, v.classes, transform=spec if s == "train" else None) for s, v in d.items()}
        if not m:
            return {s: self._split(v.x, v.y, v.classes) for s, v in d.items()} if self.u8_frames else d
        o = int(round(m / 2.0))                    # torchvision's center_crop offset
        out = {s: self._split(v.x[:, :, o:o + self.hw, o:o + self.hw], v.y, v.classes) for s, v in d.items()}
        if rnd_transform:
            out["train"] = self._split(d["train"].x, d["train"].y, d["train"].classes,
                                       transform=(RandomResizedCropFlip if self.rnd_resized else RandomCropFlip)((self.hw, self.hw)))
        return out

    def get_task_dataset_path(self, task_name=None, rnd_transform=False):
        """Task files are cached under root/name/; a sidecar task_N.spec.json records what they were generated from.  A cached
        file of ANOTHER spec (other kind / blobs / noise / sizes / seed under the same results root) is an error, not a hit:
        the results tree beside it holds success tokens and models of that other data.
        task_name=None asks for a pre-merged file of ALL tasks (Joint.grid_datafetch, method.py:1204): there is none.
        With a margin (rnd_margin or rnd_resized) or rnd_pad, rnd_transform (or rnd_always) selects task_N_rndtrans.pth.tar, which has its own sidecar."""
        if task_name is None:
            return None
        rnd = bool(self.rnd_margin or self.rnd_resized or self.rnd_pad) and (bool(rnd_transform) or self.rnd_always)
        stem = "task_%s%s" % (task_name, "_rndtrans" if rnd else "")
        path = os.path.join(self.root, self.name, stem + ".pth.tar")
        side = os.path.join(self.root, self.name, stem + ".spec.json")
        want = self.spec(task_name, rnd)
        if os.path.exists(path) and os.path.exists(side):
            with open(side) as f:
                have = json.load(f)
            if have != want:
                raise RuntimeError("%s was generated from %s, this run asks for %s: use a fresh --results_root (its results tree "
                                   "belongs to the other data)" % (path, have, want))
            return path
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if os.path.exists(path) and not os.path.exists(side):
            # data without its spec (a cache older than the sidecars, or a writer that died between the two files): regenerating is
            # only safe while no results tree (the driver keeps <results_root>/train and /test beside <results_root>/data) was
            # built from the old bytes
            if any(os.path.isdir(os.path.join(os.path.dirname(self.root), d)) for d in ("train", "test")):
                raise RuntimeError("%s has no %s beside it but a results tree exists under %s: cannot tell what data those results "
                                   "were made from — use a fresh --results_root" % (path, os.path.basename(side), os.path.dirname(self.root)))
        d = self._make(task_name, rnd)
        tmp = "%s.tmp.%d" % (path, os.getpid())    # (torch.save is not atomic: a killed writer must not leave a truncated task file)
        torch.save(d, tmp)
        os.replace(tmp, path)
        tmp = "%s.tmp.%d" % (side, os.getpid())
        with open(tmp, "w") as f:
            json.dump(want, f)
        os.replace(tmp, side)                      # written last: a data file without a sidecar is never a hit
        return path
