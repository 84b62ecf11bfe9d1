"""CPU restatement (torch, any float dtype) of the PathNet parameter kernels of csrc/pathnet.hip and of the step
PathEngine builds from them: pack the N modules of every layer of a path into one padded narrow net, run it, fold the
packed gradient back onto the modules, clip_grad_norm + momentum SGD over the active slots.  `direct_forward` is
vgg_pathnet.Net.forward itself (sum over modules), for comparison with the packed net."""
import torch
import torch.nn.functional as F


def _pad(n, g):
    return (n + g - 1) // g * g


def layers(state):
    """[dict(kind, l, M, c_out, c_in, R, ks)] in plan order, the head last (M = 1), from a vgg_pathnet.Net state dict."""
    out = []
    for kind in ("convs", "fcs"):
        l = 0
        while "%s.%d.0.weight" % (kind, l) in state:
            M = 0
            while "%s.%d.%d.weight" % (kind, l, M) in state:
                M += 1
            w = state["%s.%d.0.weight" % (kind, l)]
            out.append(dict(kind=kind, l=l, M=M, c_out=w.shape[0], shape=tuple(w.shape)))
            l += 1
    nc = sum(1 for d in out if d["kind"] == "convs")
    for i, d in enumerate(out):
        s = d["shape"]
        if d["kind"] == "convs":
            d["c_in"], d["R"], d["ks"] = s[1], s[2] * s[3], s[2]
        else:
            d["c_in"] = out[i - 1]["c_out"]
            d["R"], d["ks"] = s[1] // d["c_in"], 0
    hw = state["classifier.0.weight"]
    out.append(dict(kind="head", l=0, M=1, c_out=hw.shape[0], c_in=hw.shape[1], R=1, ks=0, shape=tuple(hw.shape)))
    return out, nc


def names(d, mod):
    if d["kind"] == "head":
        return "classifier.0.weight", "classifier.0.bias"
    return "%s.%d.%d.weight" % (d["kind"], d["l"], mod), "%s.%d.%d.bias" % (d["kind"], d["l"], mod)


def trainable(best_path, t, path, M):
    """unfreeze_path: per layer the set of modules in path[l] and not in bestPath[0:t, l, :][0]."""
    out = []
    for l, row in enumerate(path):
        bp = set(int(v) for v in best_path[0:t, l, :][0]) if t > 0 else set()
        out.append(set(int(i) for i in row if 0 <= int(i) < M and int(i) not in bp))
    return out


def pack(state, path, N, granule=32):
    """[(Wp, bp)] per layer (+ head): Wp[n*c_out+k][m*c_in+j][r] = mod[path[l][n]].w[k][j][r], zero padded to the granule;
    a slot with path < 0 stays zero.  Bitwise copies."""
    lay, nc = layers(state)
    out, prev_Kp = [], None
    for li, d in enumerate(lay):
        head = d["kind"] == "head"
        c_out, c_in, R = d["c_out"], d["c_in"], d["R"]
        n_out = 1 if head else N
        n_in = 1 if li == 0 else N
        Kp = c_out if head else _pad(N * c_out, granule)
        Cp = c_in if li == 0 else prev_Kp
        w0 = state[names(d, 0)[0]]
        Wp = torch.zeros((Kp, Cp, R), dtype=w0.dtype)
        bp = torch.zeros(Kp, dtype=w0.dtype)
        for n in range(n_out):
            mod = 0 if head else int(path[li][n])
            if mod < 0:
                continue
            wn, bn = names(d, mod)
            w = state[wn].reshape(c_out, c_in, R)
            for m in range(n_in):
                Wp[n * c_out:(n + 1) * c_out, m * c_in:(m + 1) * c_in] = w
            bp[n * c_out:(n + 1) * c_out] = state[bn]
        out.append((Wp.reshape(Kp, Cp, d["ks"], d["ks"]) if d["kind"] == "convs" else Wp.reshape(Kp, Cp * R), bp))
        prev_Kp = Kp
    return out


def forward(packed, x, maxpool_idxs, pool=(2, 2)):
    """The plain narrow net over the packed weights."""
    for li, (w, b) in enumerate(packed):
        if w.dim() == 4:
            x = F.relu(F.conv2d(x, w, b, padding=w.shape[2] // 2))
            if li in maxpool_idxs:
                x = F.max_pool2d(x, pool[0], pool[1])
        else:
            x = x.reshape(x.shape[0], -1)
            x = F.linear(x, w, b)
            if li < len(packed) - 1:
                x = F.relu(x)
    return x


def direct_forward(state, x, path, N, maxpool_idxs, pool=(2, 2)):
    """vgg_pathnet.Net.forward (vgg_pathnet.py:99-128) in eval mode; a slot of -1 contributes nothing."""
    lay, nc = layers(state)
    for li, d in enumerate(lay[:-1]):
        if d["kind"] == "fcs" and x.dim() == 4:
            x = x.reshape(x.shape[0], -1)
        acc = None
        for n in range(N):
            if int(path[li][n]) < 0:                       # an empty slot of a path recorded before N grew
                continue
            wn, bn = names(d, int(path[li][n]))
            if d["kind"] == "convs":
                y = F.relu(F.conv2d(x, state[wn], state[bn], padding=d["ks"] // 2))
                if li in maxpool_idxs:
                    y = F.max_pool2d(y, pool[0], pool[1])
            else:
                y = F.relu(F.linear(x, state[wn], state[bn]))
            acc = y if acc is None else acc + y
        x = acc
    return F.linear(x, state["classifier.0.weight"], state["classifier.0.bias"])


def active(state, path, N, train):
    """[(layer index, module)] that fold and step touch (trainable and in the first N columns), the head last."""
    lay, _ = layers(state)
    out = []
    for li, d in enumerate(lay[:-1]):
        for mod in range(d["M"]):
            if mod in train[li] and mod in [int(v) for v in path[li][:N]]:
                out.append((li, mod))
    out.append((len(lay) - 1, 0))
    return out


def fold(pgrads, state, path, N, train, dtype=None):
    """{name: gradient} of the active slots: g[mod][k][j][r] = sum_{n: path[n]==mod} sum_m G[n*c_out+k][m*c_in+j][r], summed
    n then m ascending in `dtype` (default: the dtype of the packed gradient)."""
    lay, _ = layers(state)
    out = {}
    for li, mod in active(state, path, N, train):
        d = lay[li]
        head = d["kind"] == "head"
        c_out, c_in, R = d["c_out"], d["c_in"], d["R"]
        Gw, Gb = pgrads[li]
        dt = dtype or Gw.dtype
        G3 = Gw.reshape(Gw.shape[0], -1, R).to(dt)
        gw = torch.zeros((c_out, c_in, R), dtype=dt)
        gb = torch.zeros(c_out, dtype=dt)
        n_in = 1 if li == 0 else N
        for n in range(1 if head else N):
            if not head and int(path[li][n]) != mod:
                continue
            for m in range(n_in):
                gw = gw + G3[n * c_out:(n + 1) * c_out, m * c_in:(m + 1) * c_in]
            gb = gb + Gb[n * c_out:(n + 1) * c_out].to(dt)
        wn, bn = names(d, mod)
        out[wn], out[bn] = gw.reshape(d["shape"]), gb
    return out


def clip_sgd(state, grads, bufs, lr, momentum, wd, clipgrad, first):
    """torch.nn.utils.clip_grad_norm(active, clipgrad) then torch.optim.SGD(momentum, weight_decay) over `grads`' names, in
    place on state / bufs.  Returns the total norm."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values()))
    coef = float(clipgrad) / (float(total) + 1e-6)
    coef = min(coef, 1.0)
    for n, g in grads.items():
        g = g * coef + wd * state[n]
        bufs[n] = g.clone() if first else bufs[n] * momentum + g
        state[n] = state[n] - lr * bufs[n]
    return float(total)


def train_steps(state, path, N, train, maxpool_idxs, batches, lr, momentum, wd, clipgrad, granule=32):
    """The step PathEngine runs (pack, CE over the packed net, fold, clip + SGD) for every batch; returns the new state."""
    state = {k: v.clone() for k, v in state.items()}
    bufs, first = {}, True
    for x, y in batches:
        packed = [(w.requires_grad_(True), b.requires_grad_(True)) for w, b in pack(state, path, N, granule)]
        loss = F.cross_entropy(forward(packed, x, maxpool_idxs), y)
        loss.backward()
        grads = fold([(w.grad, b.grad) for w, b in packed], state, path, N, train)
        clip_sgd(state, grads, bufs, lr, momentum, wd, clipgrad, first)
        first = False
    return state


# ------------------------------------------------------------------ comparison with the G38 fixture
# The HAT step test compares the same engine and loss with its fixture at these tolerances (test_hat_step_golden_g8:
# logits and loss 2e-4, parameters 5e-4 of the tensor's largest entry).  A parameter UPDATE is lr * (momentum-weighted
# gradients), each gradient asserted there at 5e-4 of its tensor's scale; over the three steps of the fixture => 2e-3.
TOL_LOGITS, TOL_LOSS, TOL_PARAM, TOL_DELTA = 2e-4, 2e-4, 5e-4, 2e-3


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def assert_matches_g38(g, case, logits, loss, after, start):
    """logits / loss of the first batch and the parameters after the epoch against the fixture; parameters the reference
    did not move must be bitwise the start values.  The figures are printed before they are asserted."""
    e_log, e_loss = rel(logits, g[case + "_logits"]), rel(loss, g[case + "_loss"])
    print("%s: logits %.2e loss %.2e (reference fp32 vs fp64: %s)" % (case, e_log, e_loss, g[case + "_gap"]))
    moved = [str(n) for n in g[case + "_moved"]]
    e_p = max(rel(after[n], g[case + "_p_" + n]) for n in moved)
    e_d = max(rel(after[n].double() - start[n].double(),
                  torch.from_numpy(g[case + "_p_" + n]).double() - start[n].double()) for n in moved)
    print("%s: parameters %.2e updates %.2e" % (case, e_p, e_d))
    assert e_log <= TOL_LOGITS and e_loss <= TOL_LOSS
    assert e_p <= TOL_PARAM and e_d <= TOL_DELTA
    for n in g[case + "_unmoved"]:
        assert torch.equal(after[str(n)], start[str(n)]), n
