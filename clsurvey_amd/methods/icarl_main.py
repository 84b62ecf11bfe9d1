"""iCaRL trainer on the HIP path — mirror of src/methods/rehearsal/main_rehearsal.py:main for method 'icarl' (:140-255):
argument handling, loaders at the original batch size and the batch split with the full-memory ratio, scratch wrap or
load of the IcarlNet wrapper, postprocess = manage_memory (exemplar herding) + save, else the shared rehearsal training loop
(gem_main.train_model, which dispatches observe / observe_FT)."""
import argparse
import os

import torch

from ..data import DeviceLoader, load_task_datasets
from . import gem_main
from . import icarl as I


def main(overwrite_args, nc_per_task, device="cuda"):
    """main_rehearsal.py:69-255 for method 'icarl'.  Returns (model, best validation accuracy), (None, None) after a
    postprocess."""
    parser = argparse.ArgumentParser()
    for name, kw in (("--task_name", dict(type=str)), ("--task_count", dict(type=int)),
                     ("--prev_model_path", dict(type=str)), ("--save_path", dict(type=str, default="results/")),
                     ("--n_outputs", dict(type=int, default=200)), ("--method", dict(type=str, default="icarl")),
                     ("--postprocess", dict(action="store_true")), ("--weight_decay", dict(type=float, default=0)),
                     ("--is_scratch_model", dict(action="store_true")), ("--n_memories", dict(type=int, default=0)),
                     ("--memory_strength", dict(default=0, type=float)), ("--finetune", dict(action="store_true")),
                     ("--n_epochs", dict(type=int, default=1)), ("--batch_size", dict(type=int, default=70)),
                     ("--lr", dict(type=float, default=1e-3)), ("--n_tasks", dict(type=int, default=10))):
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
    args.dset_loaders = {x: DeviceLoader(dsets[x], args.batch_size, True, device) for x in ["train", "val"]}
    dset_sizes = {x: len(dsets[x]) for x in ["train", "val"]}
    in_shape = tuple(args.dset_loaders["train"].x.shape[1:])
    step_rows = gem_main.exemplar_split(args, dset_sizes)          # :188-202: 'icarl' takes the full-memory ratio

    if args.is_scratch_model:
        assert args.task_idx == 0
        raw = torch.load(args.prev_model_path, weights_only=False)
        model = I.IcarlNet(raw, args.n_outputs, args.n_tasks, args.nc_per_task, args.n_memories, args.lr, args.weight_decay,
                           args.memory_strength, step_rows, in_shape, device)
    else:
        model = torch.load(args.prev_model_path, weights_only=False)
        if model.batch_size < step_rows:
            model.batch_size = step_rows
            model._bind()
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
