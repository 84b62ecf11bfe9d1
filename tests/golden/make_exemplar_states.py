"""Generator of exemplar_state_{gem,rehearsal,icarl}.pt: what __getstate__ of GemNet / RehearsalNet / IcarlNet returns for a
2-task wrapper over a 3x8x8 store (tensors and net on the CPU, device as a string).  Run once on a GPU machine with the
commit BEFORE methods/exemplar.py existed; tests/test_exemplar_cpu.py holds later wrappers to these key sets.
python tests/golden/make_exemplar_states.py OUT_DIR [--cpu]

--cpu: no device.  The wrappers are built on the CPU with the engine part of _bind left out (IcarlNet.fc_first, the one
pickled attribute _bind sets, is taken from the parsed plan) and the two tasks are written into the stores by the
wrappers' own host-side memory code instead of training steps: the same keys, the stores filled with random rows.
The files in this folder were made with --cpu."""
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_net():
    from clsurvey_amd.models import VGGSlim
    return VGGSlim(cfg=[8, "M", 16, "M"], num_classes=4, classifier_inputdim=16 * 2 * 2, classifier_dim1=32, classifier_dim2=32,
                   dropout=True, batch_norm=False)


def cpu_state(w):
    state = w.__getstate__()
    for k, v in list(state.items()):
        if torch.is_tensor(v) or isinstance(v, torch.nn.Module):
            state[k] = v.cpu()
    state["device"] = str(state["device"])
    return state


def main_cpu(out):
    from clsurvey_amd import net as N
    from clsurvey_amd.methods.gem import GemNet, extend_head
    from clsurvey_amd.methods.icarl import IcarlNet
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    torch.manual_seed(1)
    shape = (3, 8, 8)

    def fc_first(self):
        self.fc_first = next(i for i, sp in enumerate(N.parse_net(self.net)[0]) if sp[0] == "fc")
    GemNet._bind = RehearsalNet._bind = lambda self: None
    IcarlNet._bind = fc_first
    gem = GemNet(extend_head(make_net(), 8), 8, 2, [4, 4], 3, lr=0.01, batch_size=4, in_shape=shape, device="cpu")
    reh = RehearsalNet(replace_head(make_net(), 8), 8, 2, [4, 4], 3, 0.01, 0.0, False, 6, shape, "cpu")
    reh.init_setup(lr=0.01, weight_decay=0.0, n_append=2, chunk_size=2)
    for t in (0, 1):
        x, y = torch.randn((4,) + shape), torch.randint(0, 4, (4,))
        gem.init_new_task(t)
        gem.fill_buffer(t, x, y)
        reh.switch_task(t)
        row0, eff = reh.ring_update(t, 4)
        reh.store_x[row0:row0 + eff], reh.store_y[row0:row0 + eff] = x[:eff], y[:eff]
    reh.last_path = "fused"
    ica = IcarlNet(make_net(), 8, 2, [4, 4], 4, 0.01, 0.0, 1.0, 6, shape, "cpu")
    ica.init_setup(lr=0.01, weight_decay=0.0, memory_strength=1.0, n_append=2, chunk_size=2, total_batch_size=4)
    ica.observed_tasks, ica.old_task, ica.last_path = [0, 1], 1, "fused"
    ica.exemplar_count, ica.class_len = 1, [1] * 8                  # K/m = 8 / 8 after the second manage_memory
    ica.store_x[:8], ica.store_t[:8] = torch.randn((8,) + shape), torch.randn(8, 8)
    os.makedirs(out, exist_ok=True)
    for name, w in (("gem", gem), ("rehearsal", reh), ("icarl", ica)):
        torch.save(cpu_state(w), os.path.join(out, "exemplar_state_%s.pt" % name))
        print(name, sorted(cpu_state(w)))


def main(out):
    from clsurvey_amd.data import TensorTaskDataset
    from clsurvey_amd.methods.gem import GemNet, extend_head
    from clsurvey_amd.methods.icarl import IcarlNet
    from clsurvey_amd.methods.rehearsal import RehearsalNet, replace_head
    torch.manual_seed(1)
    random.seed(2)
    np.random.seed(3)
    shape = (3, 8, 8)

    def batch(n):
        return torch.randn((n,) + shape, device="cuda"), torch.randint(0, 4, (n,), device="cuda")
    gem = GemNet(extend_head(make_net(), 8), 8, 2, [4, 4], 3, lr=0.01, batch_size=4, in_shape=shape)
    for t in (0, 1):
        x, y = batch(4)
        gem.observe(x, t, y)
    reh = RehearsalNet(replace_head(make_net(), 8), 8, 2, [4, 4], 3, 0.01, 0.0, False, 6, shape)
    x, y = batch(4)
    reh.observe_FT(x, 0, y)
    reh.init_setup(lr=0.01, weight_decay=0.0, n_append=2, chunk_size=2)
    reh.observe_FT(x, 1, y)
    ica = IcarlNet(make_net(), 8, 2, [4, 4], 4, 0.01, 0.0, 1.0, 6, shape)
    for t in (0, 1):
        xs = torch.randn((12,) + shape, device="cuda")
        ys = torch.arange(12, device="cuda") % 4
        if t:
            ica.init_setup(lr=0.01, weight_decay=0.0, memory_strength=1.0, n_append=2, chunk_size=2, total_batch_size=4)
            ica.observe(x, t, y)
        ica.manage_memory(t, types.SimpleNamespace(task_imgfolders={"train": TensorTaskDataset(xs, ys, [])}, batch_size=4))
    torch.cuda.synchronize()
    os.makedirs(out, exist_ok=True)
    for name, w in (("gem", gem), ("rehearsal", reh), ("icarl", ica)):
        torch.save(cpu_state(w), os.path.join(out, "exemplar_state_%s.pt" % name))
        print(name, sorted(cpu_state(w)))


if __name__ == "__main__":
    (main_cpu if "--cpu" in sys.argv else main)(sys.argv[1])
