"""PathNet without a GPU: the CPU restatement tests/pathnet_ref.py against the reference's recorded forward / train_epoch
(G38), the PathNet module tree and trainable sets against the same fixture, growing N, and the argument checks of the
three entry points of csrc/pathnet.hip (nothing is launched: the pointers are dummies)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import g38_common as G  # noqa: E402
import pathnet_ref as PR  # noqa: E402

EINVAL = -1
MAXPOOL = [0, 1, 3, 5]                         # conv indices followed by "M" in G.CFG
rel = PR.rel


def start_state(setting, dtype=torch.float32):
    return {n: torch.from_numpy(v).to(dtype) for n, v in G.start_weights(setting).items()}


def best_path(case):
    c = G.CASES[case]
    N, _ = G.SETTINGS[c["setting"]]
    bp = -1 * np.ones((G.NTASKS, G.LAYERS, N), dtype=int)
    if c["best0"] is not None:
        bp[0] = np.array(c["best0"])
    return bp


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_pathnet_ref_reproduces_g38(golden, case):
    g = golden("G38_pathnet_step")
    c = G.CASES[case]
    N, M = G.SETTINGS[c["setting"]]
    path = np.array(c["path"])
    state = start_state(c["setting"], torch.float64)
    data = [(torch.from_numpy(x).double(), torch.from_numpy(y)) for x, y in G.batches(case)]
    packed = PR.pack(state, path, N)
    logits = PR.forward(packed, data[0][0], MAXPOOL)
    assert rel(logits, PR.direct_forward(state, data[0][0], path, N, MAXPOOL)) <= 1e-12
    loss = torch.nn.functional.cross_entropy(logits, data[0][1])
    train = PR.trainable(best_path(case), c["t"], path, M)
    after = PR.train_steps(state, path, N, train, MAXPOOL, data, G.LR, G.MOMENTUM, G.WD, c["clipgrad"])
    PR.assert_matches_g38(g, case, logits, loss.view(1), {k: v.float() for k, v in after.items()}, start_state(c["setting"]))


def test_pack_pads_with_zeros_and_copies_bitwise():
    state = start_state("b")
    path = np.array(G.CASES["b_dup"]["path"])
    packed = PR.pack(state, path, 3)
    w, b = packed[1]                              # 6 channels per module, 18 packed, padded to 32
    assert tuple(w.shape) == (32, 32, 3, 3) and float(w[18:].abs().max()) == 0 and float(w[:, 18:].abs().max()) == 0
    assert float(b[18:].abs().max()) == 0
    for n in range(3):
        for m in range(3):
            assert torch.equal(w[6 * n:6 * n + 6, 6 * m:6 * m + 6], state["convs.1.%d.weight" % path[1][n]])
    skip = path.copy()
    skip[2][1] = -1                               # an empty slot contributes nothing
    w, b = PR.pack(state, skip, 3)[2]
    assert float(w[6:12].abs().max()) == 0 and float(b[6:12].abs().max()) == 0 and float(w[:6].abs().max()) > 0


def _raw():
    from clsurvey_amd import models
    return models.VGGSlim(cfg=G.CFG, num_classes=G.NCLS, classifier_inputdim=64 * 2 * 2, classifier_dim1=G.FC[0],
                          classifier_dim2=G.FC[1])


def _net(setting):
    from clsurvey_amd.methods import pathnet as PN
    N, M = G.SETTINGS[setting]
    return PN.PathNet(_raw(), (3, G.HW, G.HW), [(t, G.NCLS) for t in range(G.NTASKS)], [N, M])


@pytest.mark.parametrize("setting", sorted(G.SETTINGS))
def test_pathnet_tree_is_the_reference_s(setting):
    N, M = G.SETTINGS[setting]
    net = _net(setting)
    own = [(n, tuple(p.shape)) for n, p in net.named_parameters() if not n.startswith("initial_model.")]
    assert own == G.shapes(N, M)
    assert [n for n, _ in net.named_parameters() if n.startswith("initial_model.")] == ["initial_model." + n for n, _ in own]
    assert net.bestPath.shape == (G.NTASKS, G.LAYERS, N) and (net.bestPath == -1).all() and net.bestPath.dtype.kind == "i"
    assert (net.L, net.N, net.M, net.ntasks, net.maxpool_idxs, net.smid) == (G.LAYERS, N, M, G.NTASKS, MAXPOOL, 2)
    assert [p.data_ptr() for p in net.own_parameters()] == [p.data_ptr() for n, p in net.named_parameters()
                                                            if not n.startswith("initial_model.")]


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_trainable_set_matches_what_moved_in_g38(golden, case):
    """unfreeze_path freezes the FIRST task's best path only (bestPath[0:t, l, :][0]); the head always trains."""
    g = golden("G38_pathnet_step")
    c = G.CASES[case]
    net = _net(c["setting"])
    net.bestPath = best_path(case)
    train = net.trainable_modules(c["t"], np.array(c["path"]))
    want = []
    kinds = ["convs.%d" % i for i in range(6)] + ["fcs.%d" % i for i in range(2)]
    for l, k in enumerate(kinds):
        for m in sorted(train[l]):
            want += ["%s.%d.weight" % (k, m), "%s.%d.bias" % (k, m)]
    want += ["classifier.0.weight", "classifier.0.bias"]
    assert sorted(want) == sorted(str(n) for n in g[case + "_moved"])


def test_first_task_only_is_frozen_and_growing_n_extends_best_path():
    net = _net("a")
    net.bestPath[0] = np.array(G.A_PLAIN)
    net.bestPath[1] = np.array(G.CASES["a_t1"]["path"])
    train = net.trainable_modules(2, np.array(G.CASES["a_dup"]["path"]))     # t = 2: task 1's best path is NOT frozen
    assert train[0] == {1, 3} - {0, 2} and train[1] == {2} and train[6] == {3}
    net.extend_bestPath(3)
    assert net.N == 3 and net.bestPath.shape == (G.NTASKS, G.LAYERS, 3)
    assert (net.bestPath[0, :, :2] == np.array(G.A_PLAIN)).all() and (net.bestPath[:, :, 2] == -1).all()
    assert net.trainable_modules(1, net.bestPath[1])[0] == {1}               # -1 names no module
    with pytest.raises(ValueError):
        net.extend_bestPath(2)
    state = {n: p.detach() for n, p in net.named_parameters() if not n.startswith("initial_model.")}
    wide = PR.pack(state, net.bestPath[0], 3)                                # the -1 slot packs to zero rows
    narrow = PR.pack(state, net.bestPath[0][:, :2], 2)
    assert torch.equal(wide[0][0][:16], narrow[0][0][:16]) and float(wide[0][0][16:].abs().max()) == 0
    x = torch.from_numpy(G.batches("a_plain")[0][0])
    with torch.no_grad():
        assert rel(PR.forward(wide, x, MAXPOOL), PR.forward(narrow, x, MAXPOOL)) <= 1e-6


def test_unsupported_models_are_named():
    from clsurvey_amd.methods import pathnet as PN
    import torch.nn as nn

    class AlexNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.features, self.classifier = nn.Sequential(nn.Conv2d(3, 8, 3)), nn.Sequential(nn.Linear(8, 4))
    with pytest.raises(NotImplementedError, match="AlexNet"):
        PN.PathNet(AlexNet(), (3, 32, 32), [(0, 4)], [2, 4])
    bn = _raw()
    bn.features = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU())
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        PN.PathNet(bn, (3, 32, 32), [(0, 4)], [2, 4])


def test_pathnet_entries_reject_bad_arguments():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)

    def row(**kw):
        d = dict(w_off=0, b_off=600, pw_off=0, pb_off=5000, mod_stride=700, c_out=8, c_in=8, R=9, n_out=2, n_in=2, Kp=32, Cp=32,
                 M=4, path=(C.c_int * 8)(0, 1, -1, -1, -1, -1, -1, -1), trainable=3)
        d.update(kw)
        return (_lib.PathnetLayer * 1)(_lib.PathnetLayer(*[d[k] for k, _ in _lib.PathnetLayer._fields_]))
    big = 1 << 20
    good = row()
    need = L.clhip_pathnet_ws(good, 1)
    assert need == 4 * 8                                                        # one block per module, one double each

    def calls(t, n=1, mod=big, packed=big, theta=p, ws=p, ws_bytes=need, clip=1000.0):
        return (L.clhip_pathnet_pack_multi(t, n, theta, mod, p, packed, None),
                L.clhip_pathnet_fold_grads_multi(t, n, p, packed, theta, mod, ws, ws_bytes, None),
                L.clhip_pathnet_sgd_step(t, n, theta, p, p, mod, 0.05, 0.9, 5e-4, clip, 1, ws, ws_bytes, None))
    bad = (EINVAL, EINVAL, EINVAL)
    assert calls(None) == bad and calls(good, n=0) == bad and calls(good, n=-2) == bad and calls(good, n=25) == bad
    assert calls(good, theta=None) == bad
    for kw in (dict(c_out=0), dict(c_in=-1), dict(R=0), dict(n_out=0), dict(n_out=9), dict(n_in=0), dict(n_in=9), dict(M=0),
               dict(M=65), dict(w_off=-4), dict(b_off=-4), dict(mod_stride=-1), dict(Kp=15), dict(Cp=15),
               dict(path=(C.c_int * 8)(0, 4, -1, -1, -1, -1, -1, -1))):
        assert calls(row(**kw)) == bad, kw
        assert L.clhip_pathnet_ws(row(**kw), 1) == 0, kw
    assert calls(row(pw_off=-4))[:2] == (EINVAL, EINVAL) and calls(row(pb_off=-1))[:2] == (EINVAL, EINVAL)
    assert calls(good, mod=3 * 700 + 600 + 7) == bad                            # the last module's bias ends past the arena
    assert calls(good, packed=5000 + 31)[:2] == (EINVAL, EINVAL)                # the packed bias ends past the arena
    assert calls(good, ws=None)[1:] == (EINVAL, EINVAL) and calls(good, ws_bytes=need - 1)[1:] == (EINVAL, EINVAL)
    assert calls(good, clip=0.0)[2] == EINVAL and calls(good, clip=-1.0)[2] == EINVAL
