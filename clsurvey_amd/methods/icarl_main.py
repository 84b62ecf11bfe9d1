"""iCaRL trainer on the HIP path — mirror of src/methods/rehearsal/main_rehearsal.py:main for method 'icarl' (:140-255):
argument handling, loaders at the original batch size and the batch split with the full-memory ratio, scratch wrap or
load of the IcarlNet wrapper, postprocess = manage_memory (exemplar herding) + save, else the shared rehearsal training loop
(gem_main.train_model, which dispatches observe / observe_FT).

Augmented train splits (not in the reference's arguments): overwrite_args['exemplar_frames'] = True builds the wrapper in frame
mode (icarl.py): the store holds the split's frames, herding ranks the herding view, every replay crops afresh.  Without it an
augmented split is refused by manage_memory as before.  exemplar_resized / exemplar_dtype follow gem_main.main's rules.
overwrite_args['exemplar_pad_frames'] = True is frame mode on a split carrying a RandomPadCropFlip (RandomCrop(size, padding, fill,
padding_mode) + flip): the store holds the unpadded frames, every view and replay is a window of the padded frame."""
import argparse
import os

import torch

from ..data import ByteTaskDataset, DeviceLoader, RandomCropFlip, RandomPadCropFlip, RandomResizedCropFlip, load_task_datasets
from . import gem_main
from . import icarl as I


def _frame_arguments(args, train):
    """exemplar_frames=True: the frame arguments of IcarlNet for the train split, after gem_main.main's rules for
    exemplar_resized and exemplar_dtype.  exemplar_pad_frames=True: the same for a split carrying a RandomPadCropFlip (never
    with exemplar_resized).  Decided before a device is needed."""
    spec = getattr(train, "transform", None)
    padded = getattr(args, "exemplar_pad_frames", False)
    if padded:
        if not isinstance(spec, RandomPadCropFlip):
            raise ValueError("icarl: exemplar_pad_frames=True stores the unpadded frames of a train split carrying a "
                             "RandomPadCropFlip and replays them through it; this one carries %r" % (spec,))
        if args.exemplar_resized:
            raise ValueError("icarl: exemplar_pad_frames=True replays through a RandomPadCropFlip, exemplar_resized=True through a "
                             "RandomResizedCropFlip; a train split carries one of them")
    elif not isinstance(spec, (RandomCropFlip, RandomResizedCropFlip)):
        raise ValueError("icarl: exemplar_frames=True stores the frames of an augmented train split and replays them through its "
                         "transform; this one carries %r" % (spec,))
    resized = isinstance(spec, RandomResizedCropFlip)
    if resized and not args.exemplar_resized:
        raise NotImplementedError("icarl: exemplars are replayed with RandomCropFlip only, the train split carries %r.  Resized "
                                  "replay is opt-in: pass exemplar_resized=True (the driver's --resized_exemplars)" % (spec,))
    if args.exemplar_resized and not resized:
        raise ValueError("icarl: exemplar_resized=True replays the exemplars through the RandomResizedCropFlip of the train split; "
                         "this one carries %r" % (spec,))
    if args.exemplar_dtype not in ("float32", "uint8"):
        raise ValueError("icarl: exemplar_dtype is 'float32' or 'uint8', got %r" % (args.exemplar_dtype,))
    byte_store, byte_frames = args.exemplar_dtype == "uint8", isinstance(train, ByteTaskDataset)
    if byte_store and not byte_frames:
        raise ValueError("icarl: exemplar_dtype='uint8' stores the byte frames of a train split that is a ByteTaskDataset; this one "
                         "is a %s" % type(train).__name__)
    if byte_frames and not byte_store:
        raise NotImplementedError("icarl: the default exemplar store holds fp32 frames, the augmented train split holds byte frames; "
                                  "pass exemplar_dtype='uint8' (the driver's --u8_exemplars) for a byte exemplar store")
    frames = dict(exemplar_transform=spec, frame_shape=tuple(train.x.shape[1:]))
    if byte_store:
        frames["frame_norm"] = (train.mean, train.std)
    return frames


def _spec_kind(spec):
    """The class of frame-mode replay a spec stands for."""
    return next(k for k in (RandomPadCropFlip, RandomResizedCropFlip, RandomCropFlip) if isinstance(spec, k))


def _check_loaded(model, frames):
    """A loaded wrapper keeps the store it was built with: its kind and mode agree with this call's arguments."""
    if getattr(model, "exemplar_transform", None) is None:
        raise ValueError("icarl: exemplar_frames=True, the loaded wrapper's store holds crops (it was built without it)")
    if _spec_kind(model.exemplar_transform) is not _spec_kind(frames["exemplar_transform"]):          # padded, crop or resized
        raise ValueError("icarl: the loaded wrapper replays %r, the train split carries %r"
                         % (model.exemplar_transform, frames["exemplar_transform"]))
    if (model.frame_norm is not None) != ("frame_norm" in frames):
        raise ValueError("icarl: exemplar_dtype=%r, the loaded wrapper's exemplar store is %s"
                         % ("uint8" if "frame_norm" in frames else "float32", "uint8" if model.frame_norm is not None else "float32"))


def main(overwrite_args, nc_per_task, device="cuda"):
    """main_rehearsal.py:69-255 for method 'icarl'.  Returns (model, best validation accuracy), (None, None) after a
    postprocess.
    overwrite_args['exemplar_frames'] (default False): True stores the frames of an augmented train split and replays them through
    its transform (a split without a transform is a ValueError).  With it, overwrite_args['exemplar_resized'] = True goes with a
    RandomResizedCropFlip split (either without the other is refused) and overwrite_args['exemplar_dtype'] = 'uint8' with an
    augmented ByteTaskDataset (a byte store; 'uint8' on anything else is a ValueError).  Without exemplar_frames the other two are
    not looked at and nothing differs from the plain entry.
    overwrite_args['exemplar_pad_frames'] (default False): True is frame mode on a train split carrying a RandomPadCropFlip: the
    store holds the unpadded frames (icarl.py, padded frame mode).  It implies exemplar_frames; a split carrying anything else, or
    exemplar_resized=True with it, is a ValueError; exemplar_dtype follows the byte rules above, with a byte fill per channel on a
    ByteTaskDataset.  Without it a padded split is refused (gem_main.refuse_padded_replay) whatever the other keys say."""
    parser = argparse.ArgumentParser()
    for name, kw in (("--task_name", dict(type=str)), ("--task_count", dict(type=int)),
                     ("--prev_model_path", dict(type=str)), ("--save_path", dict(type=str, default="results/")),
                     ("--n_outputs", dict(type=int, default=200)), ("--method", dict(type=str, default="icarl")),
                     ("--postprocess", dict(action="store_true")), ("--weight_decay", dict(type=float, default=0)),
                     ("--is_scratch_model", dict(action="store_true")), ("--n_memories", dict(type=int, default=0)),
                     ("--memory_strength", dict(default=0, type=float)), ("--finetune", dict(action="store_true")),
                     ("--n_epochs", dict(type=int, default=1)), ("--batch_size", dict(type=int, default=70)),
                     ("--lr", dict(type=float, default=1e-3)), ("--n_tasks", dict(type=int, default=10)),
                     ("--exemplar_frames", dict(action="store_true")), ("--exemplar_resized", dict(action="store_true")),
                     ("--exemplar_dtype", dict(type=str, default="float32")),
                     ("--exemplar_pad_frames", dict(action="store_true"))):
        parser.add_argument(name, **kw)
    args = parser.parse_known_args([])[0]
    args.nc_per_task = nc_per_task
    for key_arg, val_arg in overwrite_args.items():
        setattr(args, key_arg, val_arg)
    if args.method != "icarl":
        raise NotImplementedError("icarl_main.main runs method 'icarl', got %r (GEM and the rehearsal baselines: "
                                  "gem_main.main)" % args.method)
    args.task_idx = args.task_count - 1
    args.n_exemplars_to_append_per_batch = 0
    assert args.n_outputs == sum(args.nc_per_task)
    assert args.n_tasks == len(nc_per_task)
    if args.task_count == 1:
        assert "SI" in args.prev_model_path, "FIRST TASK NOT STARTING FROM SCRATCH, BUT FROM SI: ONLY STORING WRAPPER " \
                                             "WITH EXEMPLARS, path = {}".format(args.prev_model_path)
        assert args.postprocess, "FIRST TASK WE DO ONLY POSTPROCESSING"
    assert os.path.isfile(args.prev_model_path), "Must specify existing prev_model_path, got: " + args.prev_model_path

    dsets = load_task_datasets(args.dataset_path, device)
    args.task_imgfolders = dsets
    if args.exemplar_pad_frames:
        args.exemplar_frames = True                                  # padded frame mode is frame mode
    else:
        gem_main.refuse_padded_replay("icarl", dsets["train"], "exemplar_pad_frames=True (the driver's --icarl_padded)")
    frames = _frame_arguments(args, dsets["train"]) if args.exemplar_frames else {}
    args.dset_loaders = {x: DeviceLoader(dsets[x], args.batch_size, True, device) for x in ["train", "val"]}
    dset_sizes = {x: len(dsets[x]) for x in ["train", "val"]}
    in_shape = tuple(args.dset_loaders["train"].x.shape[1:])
    step_rows = gem_main.exemplar_split(args, dset_sizes)          # :188-202: 'icarl' takes the full-memory ratio

    if args.is_scratch_model:
        assert args.task_idx == 0
        raw = torch.load(args.prev_model_path, weights_only=False)
        model = I.IcarlNet(raw, args.n_outputs, args.n_tasks, args.nc_per_task, args.n_memories, args.lr, args.weight_decay,
                           args.memory_strength, step_rows, in_shape, device, **frames)
    else:
        model = torch.load(args.prev_model_path, weights_only=False)
        if model.batch_size < step_rows:
            model.batch_size = step_rows
            model._bind()
    if args.exemplar_frames:
        _check_loaded(model, frames)
    elif getattr(model, "exemplar_transform", None) is not None:
        raise ValueError("icarl: the loaded wrapper's store holds frames (it was built with exemplar_frames=True); pass it again")
    model.init_setup(args)
    assert model.n_tasks == args.n_tasks, "model tasks={}, args tasks={}".format(model.n_tasks, args.n_tasks)
    assert model.n_outputs == args.n_outputs

    if args.postprocess:
        model.manage_memory(args.task_idx, args)
        os.makedirs(os.path.dirname(args.save_path), exist_ok=True)
        torch.save(model, args.save_path)
        print("SAVED POSTPROCESSED MODEL TO: {}".format(args.save_path))
        return None, None
    resume = os.path.join(args.save_path, "epoch.pth.tar")
    return gem_main.train_model(model, args, dset_sizes, resume=resume)
