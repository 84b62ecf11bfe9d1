"""GEM trainer on the HIP path — mirror of src/methods/rehearsal/main_rehearsal.py:main (argument handling,
model load / wrap, postprocess = exemplar collection for the first-task model) and
rehearsal/train_rehearsal.py:train_model (epoch / phase loop, count-based LR decay and early stop).

Per training batch: GemNet.observe (memory passes + current pass through clhip_net_loss_step_slice, one
Gram pass, host QP, projection, SGD) or observe_FT in the phase-1 grid; the rehearsal baselines' RehearsalNet.observe_FT
(rehearsal.py: one assembled pass over current batch + exemplars); validation through eval_batch.
Loss / hit counters stay on the device and are read once per phase.
"""
import argparse
import copy
import math
import os
import time

import numpy as np
import torch
from ..data import load_task_datasets

from ..data import ByteTaskDataset, DeviceLoader, RandomCropFlip, RandomPadCropFlip, RandomResizedCropFlip
from .exemplar import batch_source
from . import gem as G
from . import rehearsal as R
from .train_common import set_lr


def termination_protocol(since, best_acc, best_model, exp_dir):
    """train_rehearsal.py:35-50."""
    print("Training complete in {:.0f}s, best val Acc: {:4f}".format(time.time() - since, best_acc))
    torch.save(best_model, os.path.join(exp_dir, "best_model.pth.tar"))


def train_model(model, args, dset_sizes, resume="", save_models_mode=False, saving_freq=10):
    """train_rehearsal.py:57-199. Returns (model, best validation accuracy in [0, 1])."""
    optimizer = model.opt
    exp_dir = args.save_path
    lr = args.lr
    num_epochs = args.n_epochs
    since = time.time()
    val_beat_counts = 0
    best_acc = 0.0
    best_model = None
    start_epoch = 0
    if os.path.isfile(resume):
        checkpoint = torch.load(resume, weights_only=False)
        start_epoch = checkpoint["epoch"]
        model.net.load_state_dict(checkpoint["state_dict"])      # in place, by name: parameters and buffers
        optimizer.load_state_dict(checkpoint["optimizer"])
        best_acc, lr, val_beat_counts = checkpoint["best_acc"], checkpoint["lr"], checkpoint["val_beat_counts"]
    os.makedirs(exp_dir, exist_ok=True)
    val_stats = torch.zeros(2, dtype=torch.float64, device=model.device)
    for epoch in range(start_epoch, num_epochs):
        print("Epoch {}/{}".format(epoch, num_epochs - 1))
        for phase in ["train", "val"]:
            if phase == "train":
                optimizer, lr, continue_training = set_lr(optimizer, lr, count=val_beat_counts)
                if not continue_training:
                    termination_protocol(since, best_acc, best_model, exp_dir)
                    return model, best_acc
            running_loss = torch.zeros((), dtype=torch.float64, device=model.device)
            running_corrects = torch.zeros((), dtype=torch.float64, device=model.device)
            projected = []
            val_stats.zero_()
            loader = args.dset_loaders[phase]
            frame_mode = getattr(model, "exemplar_transform", None) is not None
            for inputs, labels in loader:
                if phase == "train":
                    # frame mode: the batch goes with its frames and sample numbers (the reference's `paths`)
                    src = {"source": batch_source(loader)} if frame_mode else {}
                    if args.finetune:
                        loss, correct = model.observe_FT(inputs, args.task_idx, labels, **src)
                    else:
                        loss, correct, batch_stats = model.observe(inputs, args.task_idx, labels, **src)
                        projected.extend(batch_stats["projected_grads"])
                    running_loss = running_loss + loss.double().sum()
                    running_corrects = running_corrects + correct
                else:
                    loss = model.eval_batch(inputs, labels, args.task_idx, val_stats)
                    running_loss = running_loss + loss.double().sum()
            if phase == "val":
                running_corrects = val_stats[1]
            epoch_loss = float(running_loss.item()) / dset_sizes[phase]      # (mean batch losses) / N, as printed by the reference
            epoch_acc = float(running_corrects.item()) / dset_sizes[phase]
            print("{} Loss: {:.4f} Acc: {:.4f}".format(phase, epoch_loss, epoch_acc))
            if projected:
                # one entry per batch, zeros included, as train_rehearsal.py:153-167 prints it; the device counters are
                # stacked and read ONCE per epoch
                dev_counts = [v for v in projected if torch.is_tensor(v)]
                host = iter(torch.stack([v.reshape(()) for v in dev_counts]).cpu().tolist()) if dev_counts else iter(())
                print("projected_grads = {}".format([int(next(host)) if torch.is_tensor(v) else int(v) for v in projected]))
                if hasattr(model, "check_qp_status"):
                    model.check_qp_status()
            if math.isnan(epoch_loss):
                print("Canceling because Nan LOSS")         # train_rehearsal.py:139-141 (checked per phase here)
                return model, best_acc
            if phase == "val":
                if epoch_acc > best_acc:
                    best_acc = epoch_acc
                    if save_models_mode:
                        torch.save(model, os.path.join(exp_dir, "best_model.pth.tar"))
                    val_beat_counts = 0
                    best_model = copy.deepcopy(model)
                    print("-> New best model")
                else:
                    val_beat_counts += 1
        if save_models_mode and epoch % saving_freq == 0:
            torch.save({"epoch": epoch + 1, "lr": lr, "val_beat_counts": val_beat_counts, "epoch_acc": epoch_acc,
                        "best_acc": best_acc, "arch": "alexnet", "model": model, "state_dict": model.net.state_dict(),
                        "optimizer": optimizer.state_dict()}, os.path.join(exp_dir, "epoch.pth.tar"))
    termination_protocol(since, best_acc, best_model, exp_dir)
    return model, best_acc


BASELINES = ("baseline_rehearsal_partial_mem", "baseline_rehearsal_full_mem")


def exemplar_split(args, dset_sizes):
    """main_rehearsal.py:187-202, AFTER the loaders were made with the original batch size (:181): n_append exemplars per
    step; args.batch_size becomes the exemplar chunk size.  Returns the rows of one step (original batch + n_append).
    (The args.debug branch, :200, cannot be reached from the framework: overwrite_args never carries debug.)"""
    if args.method == "baseline_rehearsal_partial_mem":
        n_mem_samples = args.n_memories * args.task_idx
    else:
        n_mem_samples = args.n_memories * args.n_tasks
    ratio = float(n_mem_samples) / (float(dset_sizes["train"]) + n_mem_samples)
    args.n_exemplars_to_append_per_batch = int(np.ceil(args.batch_size * ratio))
    args.total_batch_size = args.batch_size
    args.batch_size = args.batch_size - args.n_exemplars_to_append_per_batch
    print("BATCH CONSISTS OF: {} new samples, {} exemplars".format(args.batch_size, args.n_exemplars_to_append_per_batch))
    return args.total_batch_size + args.n_exemplars_to_append_per_batch


def refuse_padded_replay(who, train, switch=None):
    """A train split carrying a RandomPadCropFlip is refused by iCaRL, GEM and the rehearsal baselines unless they were asked
    for padded replay (gem_main.main's exemplar_padded, icarl_main.main's exemplar_pad_frames): by default the exemplar
    assemblies crop stored frames without padding.  switch: the caller's opt-in, named in the message.
    Decided on the split alone, before any loader or device is needed."""
    spec = getattr(train, "transform", None)
    if isinstance(spec, RandomPadCropFlip):
        raise NotImplementedError("%s: padded replay is not built: exemplars are replayed with RandomCropFlip (or, opt-in, "
                                  "RandomResizedCropFlip) only, the train split carries %r%s"
                                  % (who, spec, "" if switch is None else ".  Padded replay is opt-in: pass " + switch))


def main(overwrite_args, nc_per_task, device="cuda"):
    """main_rehearsal.py:69-255 for method 'gem' and the rehearsal baselines ('baseline_rehearsal_{partial,full}_mem').
    overwrite_args['exemplar_dtype'] (not in the reference; default 'float32'): 'uint8' stores the exemplars of an augmented byte
    train split as byte frames (exemplar.py, byte store).  overwrite_args['exemplar_resized'] (not in the reference; default
    False): True replays the exemplars through the RandomResizedCropFlip of the train split (exemplar.py, resized replay);
    without it such a split is refused.  overwrite_args['exemplar_padded'] (not in the reference; default False): True replays
    the exemplars through the RandomPadCropFlip of the train split (exemplar.py, padded replay); without it such a split is
    refused."""
    parser = argparse.ArgumentParser()
    for name, kw in (("--task_name", dict(type=str)), ("--task_count", dict(type=int)),
                     ("--prev_model_path", dict(type=str)), ("--save_path", dict(type=str, default="results/")),
                     ("--n_outputs", dict(type=int, default=200)), ("--method", dict(type=str, default="gem")),
                     ("--postprocess", dict(action="store_true")), ("--weight_decay", dict(type=float, default=0)),
                     ("--is_scratch_model", dict(action="store_true")), ("--n_memories", dict(type=int, default=0)),
                     ("--memory_strength", dict(default=0, type=float)), ("--finetune", dict(action="store_true")),
                     ("--n_epochs", dict(type=int, default=1)), ("--batch_size", dict(type=int, default=70)),
                     ("--lr", dict(type=float, default=1e-3)), ("--n_tasks", dict(type=int, default=10)),
                     ("--exemplar_dtype", dict(type=str, default="float32")),
                     ("--exemplar_resized", dict(action="store_true")),
                     ("--exemplar_padded", dict(action="store_true"))):
        parser.add_argument(name, **kw)
    args = parser.parse_known_args([])[0]
    args.nc_per_task = nc_per_task
    for key_arg, val_arg in overwrite_args.items():
        setattr(args, key_arg, val_arg)
    args.task_idx = args.task_count - 1
    args.n_exemplars_to_append_per_batch = 0
    baseline = args.method in BASELINES                              # main_rehearsal.py:152-159
    if baseline:
        args.finetune = True
        args.full_mem_mode = args.method == "baseline_rehearsal_full_mem"
    elif args.method != "gem":
        raise NotImplementedError("rehearsal method %r (iCaRL has its own entry: methods.icarl_main.main)" % args.method)
    assert args.n_outputs == sum(args.nc_per_task)
    assert args.n_tasks == len(nc_per_task)
    if not baseline and args.n_tasks > G.GemNet.MAX_TASKS:           # at construction, not in the first observe of task 65
        raise ValueError("gem: n_tasks = %d, the Gram / QP / projection kernels take at most %d tasks (CLHIP_GEM_WIDE_MAX)"
                         % (args.n_tasks, G.GemNet.MAX_TASKS))
    if args.task_count == 1 and not baseline:
        assert "SI" in args.prev_model_path, "FIRST TASK NOT STARTING FROM SCRATCH, BUT FROM SI: ONLY STORING WRAPPER " \
                                             "WITH EXEMPLARS, path = {}".format(args.prev_model_path)
        assert args.postprocess, "FIRST TASK WE DO ONLY POSTPROCESSING"
    assert os.path.isfile(args.prev_model_path), "Must specify existing prev_model_path, got: " + args.prev_model_path

    dsets = load_task_datasets(args.dataset_path)
    args.task_imgfolders = dsets
    if not args.exemplar_padded:
        refuse_padded_replay("rehearsal method %r" % (args.method,), dsets["train"])
    elif not isinstance(getattr(dsets["train"], "transform", None), RandomPadCropFlip):
        raise ValueError("rehearsal method %r: exemplar_padded=True replays the exemplars through the RandomPadCropFlip of the "
                         "train split; this one carries %r" % (args.method, getattr(dsets["train"], "transform", None)))
    resized = isinstance(getattr(dsets["train"], "transform", None), RandomResizedCropFlip)
    if resized and not args.exemplar_resized:
        # by default the exemplar wrappers replay stored frames through clhip_rehearsal_assemble_crop_flip, which does not resample
        raise NotImplementedError("rehearsal method %r: exemplars are replayed with RandomCropFlip only, the train split carries %r.  "
                                  "Resized replay is opt-in: pass exemplar_resized=True (the driver's --resized_exemplars)"
                                  % (args.method, dsets["train"].transform))
    if args.exemplar_resized and not resized:
        raise ValueError("rehearsal method %r: exemplar_resized=True replays the exemplars through the RandomResizedCropFlip of the "
                         "train split; this one carries %r" % (args.method, getattr(dsets["train"], "transform", None)))
    if args.exemplar_dtype not in ("float32", "uint8"):
        raise ValueError("rehearsal method %r: exemplar_dtype is 'float32' or 'uint8', got %r" % (args.method, args.exemplar_dtype))
    byte_store = args.exemplar_dtype == "uint8"
    byte_frames = isinstance(dsets["train"], ByteTaskDataset) and isinstance(getattr(dsets["train"], "transform", None),
                                                                             (RandomCropFlip, RandomResizedCropFlip,
                                                                              RandomPadCropFlip))
    if byte_store and not byte_frames:
        raise ValueError("rehearsal method %r: exemplar_dtype='uint8' stores the byte frames of a train split that is a "
                         "ByteTaskDataset carrying a RandomCropFlip (or, with exemplar_resized=True, a RandomResizedCropFlip; with "
                         "exemplar_padded=True, a RandomPadCropFlip); "
                         "this one is a %s with transform %r"
                         % (args.method, type(dsets["train"]).__name__, getattr(dsets["train"], "transform", None)))
    if isinstance(dsets["train"], ByteTaskDataset) and getattr(dsets["train"], "transform", None) is not None and not byte_store:
        # frame mode copies fp32 frames into an fp32 store; without a transform the store holds the fp32 crops the loader served
        raise NotImplementedError("rehearsal method %r: the default exemplar store holds fp32 frames, the augmented train split holds "
                                  "byte frames; pass exemplar_dtype='uint8' (the driver's --u8_exemplars) for a byte exemplar store"
                                  % (args.method,))
    args.dset_loaders = {x: DeviceLoader(dsets[x], args.batch_size, True, device) for x in ["train", "val"]}
    dset_sizes = {x: len(dsets[x]) for x in ["train", "val"]}
    in_shape = tuple(args.dset_loaders["train"].x.shape[1:])
    # a train split with a transform: the wrapper stores frames and re-augments them at every replay (exemplar.py)
    spec = args.dset_loaders["train"].transform
    frames = dict(exemplar_transform=spec, frame_shape=tuple(dsets["train"].x.shape[1:])) if spec is not None else {}
    if byte_store:
        frames["frame_norm"] = (dsets["train"].mean, dsets["train"].std)
    if baseline:
        step_rows = exemplar_split(args, dset_sizes)

    if baseline:
        if args.is_scratch_model:
            assert args.task_idx == 0
            raw = R.replace_head(torch.load(args.prev_model_path, weights_only=False), args.n_outputs)    # :36-41
            model = R.RehearsalNet(raw, args.n_outputs, args.n_tasks, args.nc_per_task, args.n_memories, args.lr,
                                   args.weight_decay, args.full_mem_mode, step_rows, in_shape, device, **frames)
        else:
            model = torch.load(args.prev_model_path, weights_only=False)
            if model.batch_size < step_rows:
                model.batch_size = step_rows
                model._bind()
    elif args.is_scratch_model:
        assert args.task_idx == 0
        raw = torch.load(args.prev_model_path, weights_only=False)
        raw = G.extend_head(raw, args.n_outputs)                   # gem.py:96-113
        model = G.GemNet(raw, args.n_outputs, args.n_tasks, args.nc_per_task, args.n_memories, args.lr,
                         args.weight_decay, args.memory_strength, args.batch_size, in_shape, device, **frames)
    else:
        model = torch.load(args.prev_model_path, weights_only=False)
        if model.batch_size < args.batch_size:
            model.batch_size = args.batch_size
            model._bind()
    if (getattr(model, "frame_norm", None) is not None) != byte_store:
        raise ValueError("rehearsal method %r: exemplar_dtype=%r, the loaded wrapper's exemplar store is %s"
                         % (args.method, args.exemplar_dtype, "uint8" if getattr(model, "frame_norm", None) is not None else "float32"))
    model.init_setup(args)
    assert model.n_tasks == args.n_tasks, "model tasks={}, args tasks={}".format(model.n_tasks, args.n_tasks)
    assert model.n_outputs == args.n_outputs

    if args.postprocess:
        model.manage_memory(args.task_idx, args.dset_loaders["train"])
        os.makedirs(os.path.dirname(args.save_path), exist_ok=True)
        torch.save(model, args.save_path)
        print("SAVED POSTPROCESSED MODEL TO: {}".format(args.save_path))
        return None, None
    resume = os.path.join(args.save_path, "epoch.pth.tar")
    return train_model(model, args, dset_sizes, resume=resume)
