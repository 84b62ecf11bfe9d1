"""Shared by the G38 fixture generator (reference run) and the PathNet tests: the tiny net, the (N, M) settings, the
fixed paths, the NumPy-driven start weights and inputs.  Nothing here is recorded in the fixture; both sides rebuild it."""
import numpy as np

CFG = [32, "M", 32, "M", 32, 32, "M", 64, 64, "M"]
FC = (64, 64)
HW, NCLS, NTASKS = 32, 4, 2
LAYERS = 8                                   # 6 conv + 2 fc
LR, MOMENTUM, WD = 0.01, 0.9, 5e-4
BATCHES = (40, 40, 7)                        # one train_epoch: two full batches and a ragged one
SETTINGS = {"a": (2, 4), "b": (3, 5)}        # (N, M): 8 / 16 channels per module; 6 / 12 per module, 18 / 36 packed

A_PLAIN = [[0, 2], [1, 3], [3, 0], [2, 1], [0, 1], [3, 2], [1, 0], [2, 3]]
B_PLAIN = [[0, 2, 4], [1, 3, 0], [4, 0, 2], [2, 1, 3], [0, 1, 4], [3, 2, 1], [1, 0, 4], [2, 3, 4]]
# name -> setting, task, path, bestPath[0] (t = 1), clipgrad (the generator asserts whether clipping is active)
CASES = {
    "a_plain": dict(setting="a", t=0, path=A_PLAIN, best0=None, clipgrad=1000.0, clips=False),
    "a_dup": dict(setting="a", t=0, path=[[1, 3], [2, 2], [0, 3], [1, 0], [3, 2], [0, 1], [3, 3], [2, 0]], best0=None,
                  clipgrad=2.0, clips=True),
    "a_t1": dict(setting="a", t=1, path=[[0, 1], [1, 2], [2, 3], [2, 0], [3, 1], [3, 0], [1, 3], [0, 3]], best0=A_PLAIN,
                 clipgrad=2.0, clips=True),
    "b_plain": dict(setting="b", t=0, path=B_PLAIN, best0=None, clipgrad=1000.0, clips=False),
    "b_dup": dict(setting="b", t=0, path=[[1, 1, 3], [2, 4, 2], [0, 3, 4], [1, 0, 0], [3, 2, 1], [0, 1, 4], [3, 3, 0], [2, 0, 1]],
                  best0=None, clipgrad=2.0, clips=True),
    "b_t1": dict(setting="b", t=1, path=[[0, 1, 3], [1, 2, 4], [2, 3, 4], [2, 0, 4], [3, 1, 2], [3, 0, 4], [1, 3, 2], [0, 3, 1]],
                 best0=B_PLAIN, clipgrad=1000.0, clips=False),
}


def shapes(N, M):
    """[(name, shape)] of convs / fcs / classifier in named_parameters order (vgg_pathnet.py:48-89)."""
    out, c, hw = [], 3, HW
    li = 0
    for v in CFG:
        if v == "M":
            hw //= 2
            continue
        k = int(v / M)
        for m in range(M):
            out.append(("convs.%d.%d.weight" % (li, m), (k, c, 3, 3)))
            out.append(("convs.%d.%d.bias" % (li, m), (k,)))
        c = k
        li += 1
    d = c * hw * hw
    for fi, v in enumerate(FC):
        k = int(v / M)
        for m in range(M):
            out.append(("fcs.%d.%d.weight" % (fi, m), (k, d)))
            out.append(("fcs.%d.%d.bias" % (fi, m), (k,)))
        d = k
    out.append(("classifier.0.weight", (NCLS, d)))
    out.append(("classifier.0.bias", (NCLS,)))
    return out


def start_weights(setting):
    """{name: float32 array}: kaiming-like weights (the input of a layer is a sum over N modules) and small biases."""
    N, M = SETTINGS[setting]
    gen = np.random.RandomState(380 + N)
    out = {}
    for name, shape in shapes(N, M):
        if name.endswith("weight"):
            fan_in = int(np.prod(shape[1:])) * (1 if name.startswith("convs.0.") else N)
            out[name] = (gen.standard_normal(shape) * (1.0 / fan_in) ** 0.5).astype(np.float32)
        else:
            out[name] = (gen.standard_normal(shape) * 0.05).astype(np.float32)
    return out


def batches(case):
    """[(x float32 [n,3,HW,HW], y int64 [n])] of the case's train_epoch; the first batch is also the forward input."""
    gen = np.random.RandomState(3800 + sorted(CASES).index(case))
    return [(gen.standard_normal((n, 3, HW, HW)).astype(np.float32), gen.randint(0, NCLS, size=(n,)).astype(np.int64))
            for n in BATCHES]
