"""Kernel-level parity of csrc/hat.hip: the *_multi entry points of the product path (job tables past one chunk of 40,
pointers on and one float off a 16-byte boundary, block caps that make the grid-stride loops wrap, clip / compensation /
clamp on and off) and the single-job entry points, against fp64 on the CPU from the same float32 inputs.

Bitwise where the arithmetic is one float operation (scale, back-mask, clamp, g * gate) or the same code in two kernels
(single vs multi); 2 ulp for a double sum rounded once (dgate); relative 1e-12 for double sums kept in double; the fp32-chain
rule of kernel_parity.fp32_chain_check with base 1e-6 for the SGD step, the gates and the embedding gradient.
Not covered: the `total >= 2^32` index branch of hat_scale_multi_kernel, which needs a 16 GB tensor.

Measured on one MI355X (worst over the checks of a case: device distance / float32-CPU distance from fp64, both
relative to the tensor's largest entry; every check prints a `MEASURED|...` line before it asserts, run with -s):
  hat_sgd_step_multi_against_fp64[first-step]                                    1.5e-07 / 1.1e-04
  hat_sgd_step_multi_against_fp64[second-step]                                   2.5e-07 / 3.3e-07
  hat_sgd_step_multi_against_fp64[no-momentum]                                   1.5e-07 / 1.1e-04
  hat_sgd_step_multi_against_fp64[finetune]                                      5.1e-07 / 9.3e-07
  hat_sgd_step_single_agrees_with_multi                                          1.5e-07 / 1.1e-04
  hat_gates_and_emb_grads_multi[False-False-0]                                   1.1e-07 / 1.1e-07
  hat_gates_and_emb_grads_multi[False-False-2]                                   1.2e-07 / 1.2e-07
  hat_gates_and_emb_grads_multi[False-True-0]                                    8.4e-08 / 8.4e-08
  hat_gates_and_emb_grads_multi[False-True-2]                                    1.2e-07 / 1.2e-07
  hat_gates_and_emb_grads_multi[True-False-0]                                    1.1e-07 / 1.1e-07
  hat_gates_and_emb_grads_multi[True-False-2]                                    1.2e-07 / 1.2e-07
  hat_gates_and_emb_grads_multi[True-True-0]                                     8.4e-08 / 8.4e-08
  hat_gates_and_emb_grads_multi[True-True-2]                                     1.2e-07 / 1.2e-07
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi theta n = 5         0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi grad n = 5          0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi buf n = 5           0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi theta n = 1023      0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi grad n = 1023       0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi buf n = 1023        0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi theta n = 4097      0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi grad n = 4097       0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi buf n = 4097        0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi theta n = 4198403   0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi grad n = 4198403    0
  hat_sgd_step_single_agrees_with_multi: ulp single vs multi buf n = 4198403     0
  hat_weight_grads_multi: worst dgate ulp                                        0
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from kernel_parity import HAT_BASE, Arena, bitwise_equal, fp32_chain_check, ulp_distance
from oracle import hat_ref

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _L():
    from clsurvey_amd import _lib
    return _lib, _lib.lib()


# --------------------------------------------------------------------------- HAT_SGD step
SGD_SIZES = [1, 3, 4, 5, 255, 1023, 4097]
SGD_BIG = 1024 * 256 * 16 + 4099            # past 1024 blocks x 256 threads x 16 elements: the capped grid wraps
SGD = dict(lr=0.05, wd=5e-4, s=4.0, smax=400.0, thres_cosh=6.0)
CLIP_LOW, CLIP_HIGH = 1e-4, 1e9             # below every parameter's gradient norm (asserted) / never reached


@functools.lru_cache(maxsize=None)
def sgd_table():
    """45 parameters (a second chunk of the job table); every third one has a tensor one float past a 16-byte boundary —
    theta, grad, buf, mask_back in turn, then all four — so both alignment tests of both kernels see mixed cases."""
    gen = torch.Generator().manual_seed(51)
    specs = []
    for i in range(45):
        n = SGD_BIG if i == 2 else SGD_SIZES[i % len(SGD_SIZES)]
        mis = set()
        if i % 3 == 0:
            mis = [{"theta"}, {"grad"}, {"buf"}, {"mask"}, {"theta", "grad", "buf", "mask"}][(i // 3) % 5]
        is_emb = i % 5 == 1                            # 9 embeddings over every size but the long one
        has_mask = i % 2 == 0 or "mask" in mis
        theta = torch.randn(n, generator=gen) * 0.5
        if is_emb:                                     # some |s * theta| beyond thres_cosh: 4 * 2.5 > 6
            theta[::3] = torch.sign(theta[::3]) * (2.5 + 0.5 * torch.rand(theta[::3].shape, generator=gen))
        grad = torch.randn(n, generator=gen) * 0.1
        buf = torch.randn(n, generator=gen) * 0.1
        mask = None
        if has_mask:                                   # ones, fractions, and (in the long tensors only) zeros
            mask = 0.1 + 0.9 * torch.rand(n, generator=gen)
            mask[torch.rand(n, generator=gen) < 0.3] = 1.0
            if n >= 255:
                mask[torch.rand(n, generator=gen) < 0.2] = 0.0
        specs.append(dict(n=n, mis=mis, is_emb=is_emb, theta=theta, grad=grad, buf=buf, mask=mask))
    kinds = [frozenset(s["mis"]) for s in specs if s["n"] >= 4]
    assert {frozenset({"theta"}), frozenset({"grad"}), frozenset({"buf"}), frozenset({"mask"}), frozenset()} <= set(kinds)
    assert sum(1 for s in specs if s["is_emb"]) >= 4 and any(s["mask"] is None for s in specs)
    return specs


def sgd_reference(sp, theta, grad, buf, dtype, momentum, finetune, first, clipgrad, thres_emb):
    name = "embs.weight" if sp["is_emb"] else "weight"
    mb = {name: sp["mask"].to(dtype)} if sp["mask"] is not None else {}
    th, b, g = hat_ref.hat_sgd_step(name, theta.to(dtype), grad.to(dtype), buf.to(dtype), mb, 1, SGD["s"], SGD["smax"], SGD["lr"],
                                    momentum, SGD["wd"], SGD["thres_cosh"], clipgrad, finetune, first)
    raw = th
    if sp["is_emb"] and thres_emb > 0:
        th = torch.clamp(th, -thres_emb, thres_emb)
    return th, g, b, raw


def run_sgd_multi(specs, state, momentum, finetune, first, clipgrad, thres_emb):
    """state: per parameter (theta, grad, buf) host tensors.  Returns the same after the step, and whether the gaps survived."""
    _lib, L = _L()
    arenas = {k: Arena() for k in ("theta", "grad", "buf", "mask")}
    slots = []
    for sp, (th, g, b) in zip(specs, state):
        slots.append((arenas["theta"].add(th, "theta" in sp["mis"]), arenas["grad"].add(g, "grad" in sp["mis"]),
                      arenas["buf"].add(b, "buf" in sp["mis"]),
                      arenas["mask"].add(sp["mask"], "mask" in sp["mis"]) if sp["mask"] is not None else None))
    for a in arenas.values():
        a.upload(dev())
    rows = []
    for sp, (kt, kg, kb, km) in zip(specs, slots):
        ptrs = (arenas["theta"].ptr(kt), arenas["grad"].ptr(kg), arenas["buf"].ptr(kb), arenas["mask"].ptr(km) if km is not None else None)
        for nm, p in zip(("theta", "grad", "buf", "mask"), ptrs):
            assert p is None or p % 16 == (4 if nm in sp["mis"] else 0)
        rows.append(_lib.HatParam(ptrs[0], ptrs[1], ptrs[2], ptrs[3], sp["n"], int(sp["is_emb"]), 0))
    table = (_lib.HatParam * len(rows))(*rows)
    ws = torch.zeros(L.clhip_hat_sgd_multi_ws(len(rows)), dtype=torch.uint8, device=dev())
    _lib.check(L.clhip_hat_sgd_step_multi(table, len(rows), SGD["lr"], momentum, SGD["wd"], int(finetune), SGD["s"], SGD["smax"],
                                          SGD["thres_cosh"], clipgrad, thres_emb, int(first), ws.data_ptr(), ws.numel(), _stream()),
               "clhip_hat_sgd_step_multi")
    torch.cuda.synchronize()
    for a in arenas.values():
        a.download()
    out = [(arenas["theta"].get(kt).clone(), arenas["grad"].get(kg).clone(), arenas["buf"].get(kb).clone()) for kt, kg, kb, _ in slots]
    masks_kept = all(bitwise_equal(arenas["mask"].get(km), sp["mask"]) for sp, (_, _, _, km) in zip(specs, slots) if km is not None)
    return out, all(a.gaps_untouched() for a in arenas.values()) and masks_kept


SGD_CONFIGS = {
    # momentum, finetune, first, clipgrad, thres_emb
    "first-step": (0.9, False, True, CLIP_LOW, 0.0),
    "second-step": (0.9, False, False, CLIP_HIGH, 6.0),
    "no-momentum": (0.0, False, True, CLIP_LOW, 6.0),
    "finetune": (0.9, True, False, CLIP_LOW, 0.0),
}


@functools.lru_cache(maxsize=None)
def sgd_first_step():
    specs = sgd_table()
    state = [(sp["theta"], sp["grad"], sp["buf"]) for sp in specs]
    return run_sgd_multi(specs, state, *SGD_CONFIGS["first-step"])


@pytest.mark.parametrize("config", list(SGD_CONFIGS))
def test_hat_sgd_step_multi_against_fp64(request, config):
    specs = sgd_table()
    momentum, finetune, first, clipgrad, thres_emb = SGD_CONFIGS[config]
    state = [(sp["theta"], sp["grad"], sp["buf"]) for sp in specs]
    if config == "first-step":
        out, intact = sgd_first_step()
    else:
        if config == "second-step":                    # the device's own state after the first step, fresh gradients
            state = [(th, sp["grad"], b) for sp, (th, _, b) in zip(specs, sgd_first_step()[0])]
        out, intact = run_sgd_multi(specs, state, momentum, finetune, first, clipgrad, thres_emb)
    assert intact, "the step wrote outside its tensors or into mask_back"
    worst = {"theta": (0.0, 0.0), "grad": (0.0, 0.0), "buf": (0.0, 0.0)}
    clamped = 0
    failures = []
    for i, (sp, (th0, g0, b0), (th1, g1, b1)) in enumerate(zip(specs, state, out)):
        args = (momentum, finetune, first, clipgrad, thres_emb)
        r32 = sgd_reference(sp, th0, g0, b0, torch.float32, *args)
        r64 = sgd_reference(sp, th0, g0, b0, torch.float64, *args)
        if not finetune and clipgrad == CLIP_LOW:      # "below every parameter's gradient norm": the clip really acts
            unclipped = sgd_reference(sp, th0, g0, b0, torch.float64, momentum, finetune, first, CLIP_HIGH, thres_emb)[1]
            assert float(unclipped.norm()) > 2 * CLIP_LOW, "parameter %d: gradient norm below the low clip" % i
        if sp["is_emb"] and thres_emb > 0:
            clamped += int((r64[3].abs() > thres_emb).sum())
        for what, got, k in (("theta", th1, 0), ("grad", g1, 1), ("buf", b1, 2)):
            if what == "buf" and momentum == 0.0:
                assert bitwise_equal(got, b0), "momentum 0 must leave buf alone (parameter %d)" % i
                continue
            try:
                e = fp32_chain_check(request.node.name, "%s of parameter %d (n = %d)" % (what, i, sp["n"]), got, r32[k], r64[k], HAT_BASE)
                worst[what] = max(worst[what], e)
            except AssertionError as exc:
                failures.append(str(exc))
    for what, (e_dev, e_cpu) in worst.items():
        print("MEASURED|%s|worst %s|%.3e|%.3e" % (request.node.name, what, e_dev, e_cpu))
    assert not failures, "\n".join(failures)
    if config == "second-step":
        assert clamped > 0, "no embedding entry landed outside +-thres_emb before the clamp"


def test_hat_sgd_step_single_agrees_with_multi(request):
    """clhip_hat_sgd_step on four of the parameters (first step, momentum 0.9, the low clip): one block in both entry points
    up to 4096 elements => bitwise; above, the partial sums of the norm are grouped differently => the fp32-chain rule."""
    _lib, L = _L()
    specs = sgd_table()
    momentum, finetune, first, clipgrad, _ = SGD_CONFIGS["first-step"]
    multi, _ = sgd_first_step()
    def pick(pred):
        return next(i for i, sp in enumerate(specs) if pred(sp))
    chosen = {5: pick(lambda sp: sp["n"] == 5),
              1023: pick(lambda sp: sp["n"] == 1023 and sp["is_emb"] and sp["mask"] is not None),
              4097: pick(lambda sp: sp["n"] == 4097), "big": pick(lambda sp: sp["n"] == SGD_BIG)}
    d = dev()
    ws = torch.zeros(L.clhip_hat_sgd_ws(), dtype=torch.uint8, device=d)
    for key, i in chosen.items():
        sp = specs[i]
        th, g, b = sp["theta"].to(d), sp["grad"].to(d), sp["buf"].to(d)
        mb = sp["mask"].to(d) if sp["mask"] is not None else None
        _lib.check(L.clhip_hat_sgd_step(th.data_ptr(), g.data_ptr(), b.data_ptr(), mb.data_ptr() if mb is not None else None, sp["n"],
                                        SGD["lr"], momentum, SGD["wd"], int(sp["is_emb"]), int(finetune), SGD["s"], SGD["smax"],
                                        SGD["thres_cosh"], clipgrad, int(first), ws.data_ptr(), ws.numel(), _stream()), "clhip_hat_sgd_step")
        torch.cuda.synchronize()
        got = (th.cpu(), g.cpu(), b.cpu())
        r32 = sgd_reference(sp, sp["theta"], sp["grad"], sp["buf"], torch.float32, momentum, finetune, first, clipgrad, 0.0)
        r64 = sgd_reference(sp, sp["theta"], sp["grad"], sp["buf"], torch.float64, momentum, finetune, first, clipgrad, 0.0)
        for what, k in (("theta", 0), ("grad", 1), ("buf", 2)):
            fp32_chain_check(request.node.name, "%s n = %d" % (what, sp["n"]), got[k], r32[k], r64[k], HAT_BASE)
            ulps = ulp_distance(got[k], multi[i][k])
            print("MEASURED|%s|ulp single vs multi %s n = %d|%d|0" % (request.node.name, what, sp["n"], ulps))
            if sp["n"] <= 4096:
                assert ulps == 0, "%s of parameter %d (n = %d): single and multi differ by %d ulp" % (what, i, sp["n"], ulps)


# --------------------------------------------------------------------------- weight scaling / weight gradients
KCR = [(1, 1, 1), (7, 3, 9), (16, 5, 25), (8, 6, 4), (12, 10, 16), (33, 70, 1)]
KCR_BIG = (512, 1026, 16)                    # 8404992 elements > 2048 blocks x 256 threads x 16: the capped grid wraps


def test_hat_scale_weights_multi_bitwise():
    _lib, L = _L()
    gen = torch.Generator().manual_seed(61)
    shapes = [KCR[i % len(KCR)] for i in range(43)]
    shapes[1] = KCR_BIG
    null_gate, w_off, out_off = 7, 10, 39           # (7, 3, 9) copied; (12, 10, 16) with w, (8, 6, 4) with out off by a float
    assert shapes[null_gate] == (7, 3, 9) and shapes[w_off] == (12, 10, 16) and shapes[out_off] == (8, 6, 4)
    aw, ao, ag = Arena(), Arena(), Arena()
    slots = []
    for i, (K, Cc, R) in enumerate(shapes):
        w = torch.randn(K * Cc * R, generator=gen)
        gate = torch.rand(Cc, generator=gen)
        slots.append((aw.add(w, i == w_off), ao.add(torch.full((K * Cc * R,), float("nan")), i == out_off),
                      ag.add(gate) if i != null_gate else None, w, gate))
    for a in (aw, ao, ag):
        a.upload(dev())
    layers = (_lib.HatLayer * len(shapes))(*[_lib.HatLayer(aw.ptr(kw), ag.ptr(kg) if kg is not None else None, ao.ptr(ko), K, Cc, R)
                                            for (K, Cc, R), (kw, ko, kg, _, _) in zip(shapes, slots)])
    assert aw.ptr(slots[w_off][0]) % 16 == 4 and ao.ptr(slots[out_off][1]) % 16 == 4
    _lib.check(L.clhip_hat_scale_weights_multi(layers, len(shapes), _stream()), "clhip_hat_scale_weights_multi")
    torch.cuda.synchronize()
    for a in (aw, ao, ag):
        a.download()
    assert aw.gaps_untouched() and ao.gaps_untouched() and ag.gaps_untouched()
    d = dev()
    for i, ((K, Cc, R), (kw, ko, kg, w, gate)) in enumerate(zip(shapes, slots)):
        want = w if kg is None else (w.view(K, Cc, R) * gate.view(1, Cc, 1)).reshape(-1)      # one float32 product per element
        got = ao.get(ko)
        assert bitwise_equal(got, want), "layer %d %r: %d elements differ" % (i, (K, Cc, R), int((got != want).sum()))
        assert bitwise_equal(aw.get(kw), w)
        if i in (2, 3, null_gate):                        # the single-job entry point on three layers
            out1 = torch.full((K * Cc * R,), float("nan"), device=d)
            wd, gd = w.to(d), gate.to(d)
            _lib.check(L.clhip_hat_scale_weight(wd.data_ptr(), gd.data_ptr() if kg is not None else None, out1.data_ptr(), K, Cc, R,
                                                _stream()), "clhip_hat_scale_weight")
            torch.cuda.synchronize()
            assert bitwise_equal(out1, got), "layer %d: single and multi differ" % i


def test_hat_weight_grads_multi():
    _lib, L = _L()
    gen = torch.Generator().manual_seed(62)
    shapes = [KCR[i % len(KCR)] for i in range(42)]
    assert any(c == 1 for _, c, _ in shapes) and any(k * r < 256 for k, _, r in shapes) and any(k * r > 256 for k, _, r in shapes)
    agr, aw, ag, adg = Arena(), Arena(), Arena(), Arena()
    slots = []
    for K, Cc, R in shapes:
        g = torch.randn(K * Cc * R, generator=gen)
        w = torch.randn(K * Cc * R, generator=gen)
        gate = torch.rand(Cc, generator=gen)
        slots.append((agr.add(g), aw.add(w), ag.add(gate), adg.add(torch.full((Cc,), float("nan"))), g, w, gate))
    for a in (agr, aw, ag, adg):
        a.upload(dev())
    jobs = (_lib.HatWgradJob * len(shapes))(*[_lib.HatWgradJob(agr.ptr(s[0]), aw.ptr(s[1]), ag.ptr(s[2]), adg.ptr(s[3]), K, Cc, R, 0)
                                             for (K, Cc, R), s in zip(shapes, slots)])
    _lib.check(L.clhip_hat_weight_grads_multi(jobs, len(shapes), _stream()), "clhip_hat_weight_grads_multi")
    torch.cuda.synchronize()
    for a in (agr, aw, ag, adg):
        a.download()
    assert all(a.gaps_untouched() for a in (agr, aw, ag, adg))
    d = dev()
    worst = 0
    for i, ((K, Cc, R), (kg, kw, kgate, kdg, g, w, gate)) in enumerate(zip(shapes, slots)):
        dgate64 = (g.double() * w.double()).view(K, Cc, R).sum((0, 2))
        ulps = ulp_distance(adg.get(kdg), dgate64.float())
        worst = max(worst, ulps)
        assert ulps <= 2, "job %d %r: dgate %d ulp from the rounded fp64 sum" % (i, (K, Cc, R), ulps)
        want = (g.view(K, Cc, R) * gate.view(1, Cc, 1)).reshape(-1)
        assert bitwise_equal(agr.get(kg), want), "job %d %r: g is not g_before * gate[c]" % (i, (K, Cc, R))
        assert bitwise_equal(aw.get(kw), w)
        if i in (0, 1, 2, 5):                              # the single-job entry point on copies: C = 1, K*R < and > 256, R = 1
            gd, wd, gated = g.to(d), w.to(d), gate.to(d)
            dw = torch.full((K * Cc * R,), float("nan"), device=d)
            dg = torch.full((Cc,), float("nan"), device=d)
            _lib.check(L.clhip_hat_weight_grad(gd.data_ptr(), wd.data_ptr(), gated.data_ptr(), dw.data_ptr(), dg.data_ptr(), K, Cc, R,
                                               _stream()), "clhip_hat_weight_grad")
            torch.cuda.synchronize()
            assert bitwise_equal(dw, agr.get(kg)) and bitwise_equal(dg, adg.get(kdg)), "job %d: single and multi differ" % i
    print("MEASURED|test_hat_weight_grads_multi|worst dgate ulp|%d|0" % worst)


# --------------------------------------------------------------------------- gates / embedding gradients
GATE_N = [1, 64, 255, 256, 257, 1000]
ROWS = 3


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("t", [0, ROWS - 1])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_sums", [False, True])
def test_hat_gates_and_emb_grads_multi(request, t, with_mask, with_sums):
    _lib, L = _L()
    case = request.node.name
    d = dev()
    gen = torch.Generator().manual_seed(71)
    s, lamb = 7.5, 0.75
    embs = [torch.randn((ROWS, n), generator=gen) for n in GATE_N]
    masks = []
    for li, n in enumerate(GATE_N):                      # with_mask: zeros, ones and fractions; one layer keeps a NULL mask
        m = None
        if with_mask and li != 3:
            m = torch.rand(n, generator=gen)
            m[torch.rand(n, generator=gen) < 0.3] = 0.0
            m[torch.rand(n, generator=gen) < 0.3] = 1.0
        masks.append(m)
    dgates = [torch.randn(n, generator=gen) * 0.1 for n in GATE_N]
    embs_d = [e.to(d) for e in embs]
    masks_d = [m.to(d) if m is not None else None for m in masks]
    gates_d = [torch.full((n,), float("nan"), device=d) for n in GATE_N]
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=d) if with_sums else None
    jobs = (_lib.HatGateJob * len(GATE_N))(*[_lib.HatGateJob(e[t].data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else None, n, 0)
                                            for e, g, m, n in zip(embs_d, gates_d, masks_d, GATE_N)])
    _lib.check(L.clhip_hat_gates_multi(jobs, len(GATE_N), s, sums.data_ptr() if with_sums else None, _stream()), "clhip_hat_gates_multi")
    torch.cuda.synchronize()
    gates = [g.cpu() for g in gates_d]
    s0 = s1 = 0.0
    for e, a, m, n in zip(embs, gates, masks, GATE_N):
        fp32_chain_check(case, "gate n = %d" % n, a, torch.sigmoid(s * e[t]), torch.sigmoid(s * e[t].double()), HAT_BASE)
        aux = 1 - m if m is not None else torch.ones(n)            # float32, as the kernel forms it
        s0 += float((a * aux).double().sum())                      # the float32 product, summed in double
        s1 += float(aux.double().sum())
    if with_sums:
        got = sums.cpu().tolist()
        for k, want in enumerate((s0, s1, s0 / s1)):
            assert _rel(got[k], want) <= 1e-12, "sums[%d] = %r, fp64 %r" % (k, got[k], want)
    # single-job gate and layer-by-layer regulariser sums
    acc = torch.zeros(2, dtype=torch.float64, device=d)
    for e, a, m, n in zip(embs_d, gates, masks_d, GATE_N):
        one = torch.full((n,), float("nan"), device=d)
        _lib.check(L.clhip_hat_gate(e[t].data_ptr(), n, s, one.data_ptr(), _stream()), "clhip_hat_gate")
        _lib.check(L.clhip_hat_reg_sums(one.data_ptr(), m.data_ptr() if m is not None else None, n, acc.data_ptr(), _stream()),
                   "clhip_hat_reg_sums")
        torch.cuda.synchronize()
        assert bitwise_equal(one, a), "clhip_hat_gate and clhip_hat_gates_multi differ at n = %d" % n
    acc = acc.cpu().tolist()
    assert _rel(acc[0], s0) <= 1e-12 and _rel(acc[1], s1) <= 1e-12, (acc, s0, s1)

    # embedding gradients: count passed by the caller, and count = 0 read from sums[1] on the device
    for count in ([s1] + ([0.0] if with_sums else [])):
        dg_d = [x.to(d) for x in dgates]
        demb_d = [torch.full((ROWS, n), float("nan"), device=d) for n in GATE_N]
        ej = (_lib.HatEmbJob * len(GATE_N))(*[_lib.HatEmbJob(dg.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else None,
                                                            o.data_ptr(), n, ROWS, t, 0)
                                             for dg, g, m, o, n in zip(dg_d, gates_d, masks_d, demb_d, GATE_N)])
        _lib.check(L.clhip_hat_emb_grads_multi(ej, len(GATE_N), s, lamb, count, sums.data_ptr() if with_sums else None, _stream()),
                   "clhip_hat_emb_grads_multi")
        torch.cuda.synchronize()
        cnt32 = np.float32(s1)                                      # what the kernel divides by in both forms
        loc32 = float(np.float32(lamb) / cnt32)
        for dg, a, m, o, n, dgd, gd, md in zip(dgates, gates, masks, demb_d, GATE_N, dg_d, gates_d, masks_d):
            o = o.cpu()
            other = [r for r in range(ROWS) if r != t]
            assert bool((o[other] == 0).all()), "rows other than t must be exactly 0"
            aux = 1 - m if m is not None else torch.ones(n)
            want32 = (dg + loc32 * aux) * (s * a * (1 - a))
            a64, loc64 = a.double(), lamb / float(cnt32)
            want64 = (dg.double() + loc64 * aux.double()) * (s * a64 * (1 - a64))
            fp32_chain_check(case, "demb n = %d count = %g" % (n, count), o[t], want32, want64, HAT_BASE)
            one = torch.full((n,), float("nan"), device=d)
            _lib.check(L.clhip_hat_emb_grad(dgd.data_ptr(), gd.data_ptr(), md.data_ptr() if md is not None else None, n, s, loc32,
                                            one.data_ptr(), _stream()), "clhip_hat_emb_grad")
            torch.cuda.synchronize()
            assert bitwise_equal(one, o[t]), "clhip_hat_emb_grad and row t of clhip_hat_emb_grads_multi differ at n = %d" % n


# --------------------------------------------------------------------------- back-mask / clamp
@pytest.mark.parametrize("K,Cc,R,bias", [(7, 3, 9, False), (33, 70, 1, False), (5, 1, 1, True)])
def test_hat_backmask_bitwise(K, Cc, R, bias):
    _lib, L = _L()
    gen = torch.Generator().manual_seed(81)
    post, pre = torch.rand(K, generator=gen), torch.rand(Cc, generator=gen)
    d = dev()
    out = torch.full((K * Cc * R,), float("nan"), device=d)
    pd, qd = post.to(d), pre.to(d)
    _lib.check(L.clhip_hat_backmask(pd.data_ptr(), None if bias else qd.data_ptr(), out.data_ptr(), K, Cc, R, _stream()), "clhip_hat_backmask")
    torch.cuda.synchronize()
    v = post.view(K, 1, 1).expand(K, Cc, R)
    if not bias:
        v = torch.minimum(v, pre.view(1, Cc, 1).expand(K, Cc, R))
    assert bitwise_equal(out, (1 - v).reshape(-1))


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_clamp_bitwise(n):
    _lib, L = _L()
    x = torch.randn(n, generator=torch.Generator().manual_seed(82)) * 6
    xd = torch.cat([torch.full((4,), 99.0), x, torch.full((4,), 99.0)]).to(dev())
    _lib.check(L.clhip_clamp(xd.data_ptr() + 16, n, -6.0, 6.0, _stream()), "clhip_clamp")
    torch.cuda.synchronize()
    got = xd.cpu()
    assert bitwise_equal(got[4:4 + n], torch.clamp(x, -6.0, 6.0)) and bool((got[:4] == 99.0).all()) and bool((got[4 + n:] == 99.0).all())
