"""PathNet on the HIP path — mirror of src/methods/HAT/networks/vgg_pathnet.py (Net) and the batch step of
approaches/pathnet.py (train_epoch: CE, clip_grad_norm, torch.optim.SGD over the trainable modules).

A path (N of M modules per layer, summed behind ReLU / pool) is PACKED into the weights of a plain narrow net (see
csrc/pathnet.hip), which the ordinary NetEngine plan runs; the packed gradient is FOLDED back onto the modules.  Only the
three parameter-sized kernels are PathNet specific.
"""
import copy
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._lib import check
from ..net import NetEngine, ParamArena, conv_geometry

GRANULE = 32        # every packed width is padded with zero channels to a multiple of this (PathNet row)
MAX_N = 8           # CLHIP_PATHNET_MAX_N


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pad(n, g=GRANULE):
    return (n + g - 1) // g * g


class PathNet(nn.Module):
    """Same parameter tree as vgg_pathnet.Net (vgg_pathnet.py:18-97): convs[l][m], fcs[l][m], classifier[0], and the
    deep copy `initial_model` (a registered sub-module there as well, so its keys are part of the state dict)."""

    def __init__(self, rawmodel, inputsize, taskcla, parameter):
        super().__init__()
        if not hasattr(rawmodel, "features") or not hasattr(rawmodel, "classifier"):
            raise NotImplementedError("PathNet: the raw model needs features / classifier")
        if type(rawmodel).__name__ == "AlexNet":
            raise NotImplementedError("PathNet: AlexNet (alexnet_pathnet.py) is not built")
        if any(isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)) for m in rawmodel.modules()):
            raise NotImplementedError("PathNet: nets with BatchNorm are not built")
        ncha, size, _ = inputsize
        self.taskcla = taskcla
        self.ntasks = len(taskcla)
        self.N, self.M = int(parameter[0]), int(parameter[1])
        self.convs, self.fcs, self.classifier = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.maxpool_idxs = []
        self.pool_geometry = None    # (kernel, stride) of the raw model's first MaxPool2d: one pool module serves all (:63-67)
        self.drop_p = 0.0            # p of the raw classifier's first Dropout; 0 = none (:88-89)
        one = lambda v: v if isinstance(v, int) else v[0]
        s, conv_idx, in_channels, out_channels = size, 0, None, None
        for mod in rawmodel.features.children():
            if isinstance(mod, nn.Conv2d):
                out_channels = int(mod.out_channels / self.M)
                in_channels = mod.in_channels if in_channels is None else in_channels
                self.convs.append(nn.ModuleList(
                    nn.Conv2d(in_channels, out_channels, kernel_size=mod.kernel_size, stride=mod.stride, padding=mod.padding)
                    for _ in range(self.M)))
                in_channels = out_channels
                conv_idx += 1
            elif isinstance(mod, nn.MaxPool2d):
                if self.pool_geometry is None:
                    self.pool_geometry = (one(mod.kernel_size), one(mod.stride))
                self.maxpool_idxs.append(conv_idx - 1)
                s = int(np.floor((s - self.pool_geometry[0]) / float(self.pool_geometry[1]) + 1))     # HAT_utils.py: conv output size
        self.smid = s
        in_feats = out_channels * s * s
        linears = [m for m in rawmodel.classifier.children() if isinstance(m, nn.Linear)]
        for i, mod in enumerate(linears):
            if i < len(linears) - 1:
                out_features = int(mod.out_features / self.M)
                self.fcs.append(nn.ModuleList(nn.Linear(in_feats, out_features) for _ in range(self.M)))
                in_feats = out_features
            else:
                self.classifier.append(nn.Linear(in_feats, mod.out_features))
        for mod in rawmodel.classifier.children():
            if isinstance(mod, nn.Dropout) and self.drop_p == 0.0:
                self.drop_p = float(mod.p)
        self.L = len(self.convs) + len(self.fcs)
        self.bestPath = -1 * np.ones((self.ntasks, self.L, self.N), dtype=int)
        self.initial_model = copy.deepcopy(self)

    def own_parameters(self):
        """convs, fcs, classifier in module order: what trains (initial_model only ever supplies re-initialisations)."""
        return list(self.convs.parameters()) + list(self.fcs.parameters()) + list(self.classifier.parameters())

    def layer_modules(self):
        return list(self.convs) + list(self.fcs)

    def extend_bestPath(self, N):
        """approaches/pathnet.py:66-81 as it evidently intends (the reference builds the wider array and never assigns it):
        bestPath grows to N columns, the new slots hold -1 = no module."""
        N = int(N)
        if N < self.N:
            raise ValueError("N should only increase in the framework! {} -> {}".format(self.N, N))
        if N > self.N:
            wide = -1 * np.ones(self.bestPath.shape[:2] + (N,), dtype=int)
            wide[:, :, :self.bestPath.shape[2]] = self.bestPath
            self.bestPath = wide
        self.N = N

    def trainable_modules(self, t, path):
        """unfreeze_path (vgg_pathnet.py:130-150): module i of layer l trains iff i is in path[l] and not in
        bestPath[0:t, l, :][0] — the best path of the FIRST task only.  Returns one set per layer."""
        path = np.asarray(path)
        out = []
        for l in range(self.L):
            bp = set(int(v) for v in self.bestPath[0:t, l, :][0]) if t > 0 else set()
            out.append(set(int(i) for i in path[l] if 0 <= int(i) < self.M and int(i) not in bp))
        return out


class PathSGD:
    """The state torch.optim.SGD(momentum) keeps in approaches/pathnet.py:61-64: one momentum arena and the first-step flag."""

    def __init__(self, engine, lr, momentum=0.9, weight_decay=0.0):
        self.lr, self.momentum, self.weight_decay = float(lr), float(momentum), float(weight_decay)
        self.buf = torch.zeros_like(engine.A.theta)
        self.first = True


class PathEngine:
    """forward / step of vgg_pathnet.Net.forward(x, t, P) + approaches/pathnet.py:train_epoch for one batch."""

    def __init__(self, net, max_batch, in_shape, device="cuda"):
        if net.N > MAX_N or net.M > 64:
            raise NotImplementedError("PathEngine: N <= %d and M <= 64" % MAX_N)
        self.net = net.to(device)
        self.device = torch.device(device)
        self.A = ParamArena(net.own_parameters(), self.device)           # module arena
        self.N = net.N
        groups = net.layer_modules()
        self.nc = len(net.convs)
        # the padded plain view: one packed Conv2d / Linear per layer, widths N*c padded to the granule
        self.holder = nn.Module()
        self.holder.packed = nn.ParameterList()
        specs, drops, self._geo = [], {}, []
        pk, ps = net.pool_geometry or (2, 2)
        prev_c, prev_Kp = None, None
        for li, group in enumerate(groups):
            m0 = group[0]
            conv = li < self.nc
            c_out = m0.out_channels if conv else m0.out_features
            Kp = _pad(self.N * c_out)
            if li == 0:
                c_in, n_in, Cp, R = m0.in_channels, 1, m0.in_channels, int(m0.weight.shape[2] * m0.weight.shape[3])
            elif conv:
                c_in, n_in, Cp, R = prev_c, self.N, prev_Kp, int(m0.weight.shape[2] * m0.weight.shape[3])
            else:
                R = net.smid * net.smid if li == self.nc else 1
                c_in, n_in, Cp = prev_c, self.N, prev_Kp
            assert m0.weight.numel() == c_out * c_in * R
            if conv:
                ks = int(m0.weight.shape[2])
                w = nn.Parameter(torch.zeros(Kp, Cp, ks, ks))
            else:
                w = nn.Parameter(torch.zeros(Kp, Cp * R))
            b = nn.Parameter(torch.zeros(Kp))
            self.holder.packed.extend([w, b])
            if conv:
                pool = False
                if li in net.maxpool_idxs:
                    pool = True if (pk, ps) == (2, 2) else (pk, ps)
                specs.append(("conv", w, b, Cp, Kp, True, pool, conv_geometry(m0)))
            else:
                specs.append(("fc", w, b, Cp * R, Kp, True, False))
                if net.drop_p > 0 and li > self.nc:
                    drops[li] = nn.Dropout(net.drop_p)
            stride = self.A.slot(group[1].weight)[0] - self.A.slot(m0.weight)[0] if len(group) > 1 else 0
            assert all(self.A.slot(g.weight)[0] == self.A.slot(m0.weight)[0] + i * stride and
                       self.A.slot(g.bias)[0] == self.A.slot(m0.bias)[0] + i * stride for i, g in enumerate(group))
            self._geo.append(dict(w=m0.weight, b=m0.bias, pw=w, pb=b, stride=stride, c_out=c_out, c_in=c_in, R=R,
                                  n_out=self.N, n_in=n_in, Kp=Kp, Cp=Cp, M=len(group)))
            prev_c, prev_Kp = c_out, Kp
        head = net.classifier[0]
        w = nn.Parameter(torch.zeros(head.out_features, prev_Kp))
        b = nn.Parameter(torch.zeros(head.out_features))
        self.holder.packed.extend([w, b])
        specs.append(("fc", w, b, prev_Kp, head.out_features, False, False))
        if net.drop_p > 0:
            drops[len(groups)] = nn.Dropout(net.drop_p)
        self._geo.append(dict(w=head.weight, b=head.bias, pw=w, pb=b, stride=0, c_out=head.out_features, c_in=prev_c, R=1,
                              n_out=1, n_in=self.N, Kp=head.out_features, Cp=prev_Kp, M=1))
        self.engine = NetEngine(self.holder, max_batch, in_shape, device, layers=specs, params=list(self.holder.packed),
                                drops=drops)
        self.P = self.engine.arena                                       # packed arena
        self._table = None
        self._ws = None
        self._dirty = True
        self.path = None

    # ------------------------------------------------------------------ job table
    def set_path(self, path, t):
        """path: [L][>= N] module indices (the forward uses the first N columns, vgg_pathnet.py:108-124; -1 = empty slot);
        t: the task, for the trainable set.  Builds the job table of the three launches and packs."""
        path = np.asarray(path, dtype=int)
        if path.shape[0] != self.net.L or path.shape[1] < self.N:
            raise ValueError("PathEngine.set_path: path %s does not fit L=%d, N=%d" % (path.shape, self.net.L, self.N))
        if path.max() >= self.net.M:
            raise ValueError("PathEngine.set_path: module index beyond M")
        train = self.net.trainable_modules(t, path)
        rows = []
        for li, g in enumerate(self._geo):
            head = li == len(self._geo) - 1
            slots = [0] if head else [int(v) if v >= 0 else -1 for v in path[li, :self.N]]
            mask = 1 if head else sum(1 << i for i in train[li])
            rows.append(_lib.PathnetLayer(self.A.slot(g["w"])[0], self.A.slot(g["b"])[0], self.P.slot(g["pw"])[0],
                                          self.P.slot(g["pb"])[0], g["stride"], g["c_out"], g["c_in"], g["R"], g["n_out"],
                                          g["n_in"], g["Kp"], g["Cp"], g["M"], (C.c_int * MAX_N)(*(slots + [-1] * (MAX_N - len(slots)))),
                                          mask))
        self._table = (_lib.PathnetLayer * len(rows))(*rows)
        self.path = path
        need = _lib.lib().clhip_pathnet_ws(self._table, len(rows))
        if need == 0:
            raise _lib.ClhipError("clhip_pathnet_ws: CLHIP_EINVAL")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        self.pack()

    def active_slots(self):
        """[(layer, module)] that fold and step touch: trainable and in the first N columns of the path; the head is
        (L, 0)."""
        out = []
        for li, row in enumerate(self._table):
            for i in range(row.M):
                if (row.trainable >> i) & 1 and i in list(row.path)[:row.n_out]:
                    out.append((li, i))
        return out

    def pack(self):
        check(_lib.lib().clhip_pathnet_pack_multi(self._table, len(self._table), self.A.theta.data_ptr(), self.A.numel,
                                                  self.P.theta.data_ptr(), self.P.numel, _stream()), "clhip_pathnet_pack_multi")
        self._dirty = False

    def fold(self):
        check(_lib.lib().clhip_pathnet_fold_grads_multi(self._table, len(self._table), self.P.grad.data_ptr(), self.P.numel,
                                                        self.A.grad.data_ptr(), self.A.numel, self._ws.data_ptr(),
                                                        self._ws.numel(), _stream()), "clhip_pathnet_fold_grads_multi")

    def sgd(self, opt, clipgrad):
        check(_lib.lib().clhip_pathnet_sgd_step(self._table, len(self._table), self.A.theta.data_ptr(), self.A.grad.data_ptr(),
                                                opt.buf.data_ptr(), self.A.numel, opt.lr, opt.momentum, opt.weight_decay,
                                                float(clipgrad), int(opt.first), self._ws.data_ptr(), self._ws.numel(),
                                                _stream()), "clhip_pathnet_sgd_step")
        opt.first = False
        self._dirty = True

    # ------------------------------------------------------------------ passes
    def forward(self, x):
        """Net.forward(x, t, path) logits; packs only when the modules changed since the last pack (an evaluation pass
        packs once)."""
        if self._table is None:
            raise RuntimeError("PathEngine: set_path first")
        if self._dirty:
            self.pack()
        self.holder.training = self.net.training
        return self.engine.forward(x)

    def loss(self, x, y, stats=None, want_logits=False):
        """CE (mean) of a batch without a backward pass: (loss[1] device tensor, logits|None)."""
        if self._dirty:
            self.pack()
        self.holder.training = self.net.training
        return self.engine.loss_step(x, y, "ce_mean", False, stats, want_logits)

    def step(self, x, y, opt, clipgrad, stats=None, want_logits=False):
        """One batch of train_epoch (pathnet.py:219-227): pack, the net's own plan with CE, fold, clip + SGD.  Three launches
        next to the plan, no host synchronisation.  Returns (loss[1] device tensor, logits|None)."""
        if self._table is None:
            raise RuntimeError("PathEngine: set_path first")
        self.pack()
        self.holder.training = self.net.training
        out = self.engine.loss_step(x, y, "ce_mean", True, stats, want_logits)
        self.fold()
        self.sgd(opt, clipgrad)
        return out

    def snapshot(self):
        """HAT_utils.get_model_state on the device: a copy of the module arena."""
        return self.A.theta.clone()

    def restore(self, state):
        """HAT_utils.set_model_state_."""
        self.A.theta.copy_(state)
        self._dirty = True
