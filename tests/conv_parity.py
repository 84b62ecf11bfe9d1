"""What test_gpu_conv2d_kernels.py, test_gpu_conv5x5_bs_kernels.py, test_gpu_wino_kernels.py, test_gpu_conv3x3_kernels.py and test_gpu_bs3x3_kernels.py share (test infrastructure): operands of a convolution
layer, one raw-pointer call of an entry point on a fresh kernel_parity.Arena, and the per-element accuracy rule.

Arena layout of a call: every operand lies directly between two runs of GUARD floats that hold a NaN bit pattern (a read of even
one float in front of or behind an operand makes the result non-finite), outputs start as a second NaN pattern (an element that is never written stays non-finite), the workspace
as a third with WS_SLACK floats behind what the call is told it may use."""
import functools
import types

import pytest
import torch

from kernel_parity import Arena, ByteArena, ConvRef, all_bits, bit_pattern, bitwise_equal, ulp_distance

WS_BITS = 0x7FC0BEEF          # workspace before a call: a quiet NaN, payload 0xBEEF
OUT_BITS = 0x7FC00A11         # outputs before a call
GUARD_BITS = 0x7FC0D00D       # guard items on both sides of every operand
BYTE_OUT = 0xEE               # uint8 outputs before a call (the arg-max codes are 0..4; ByteArena's gap bytes are 0xA5)
GUARD = 80                    # NaN floats directly in front of and behind every operand (a multiple of 4)
WS_SLACK = 64                 # floats of workspace handed over beyond what a call needs
U = 2.0 ** -24                # unit roundoff of float32


def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def product_lib():
    from clsurvey_amd import _lib
    return _lib.lib()


def out_dims(shape):
    N, C, H, W, K, R, S, st, pad = shape
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def operands(shape, seed=0, positive=False):
    """x ~ N(0,1) [N][C][H][W], w ~ 0.05 N(0,1) [K][C][R][S] with out-channel 0 all zero (exact zero sums for the ReLU test),
    dy ~ N(0,1) [N][K][OH][OW]; no other zero anywhere.  positive: |.| of the same draws and no zero channel (coherent errors)."""
    N, C, H, W, K, R, S, st, pad = shape
    OH, OW = out_dims(shape)
    gen = torch.Generator().manual_seed(1000 * seed + 131 * N + 17 * C + 7 * H + 3 * W + 5 * K + 11 * R + 13 * S + st + pad)
    x, w, dy = torch.randn((N, C, H, W), generator=gen), torch.randn((K, C, R, S), generator=gen) * 0.05, torch.randn((N, K, OH, OW), generator=gen)
    assert bool((x != 0).all()) and bool((w != 0).all()) and bool((dy != 0).all())
    if positive:
        return x.abs(), w.abs(), dy.abs()
    w[0] = 0.0
    return x, w, dy


@functools.lru_cache(maxsize=None)
def reference(shape, seed=0, positive=False):
    x, w, dy = operands(shape, seed, positive)
    return ConvRef(x, w, dy, shape[7], shape[8])


def epilogue_inputs(shape):
    """bias [K] with b[0] = -0.0 (out-channel 0 has zero weights: its sums are exactly 0); relu_src [N][C][H][W] with 0.0, -0.0,
    a negative denormal, a NaN and plain negative entries planted."""
    N, C, H, W, K, R, S, st, pad = shape
    gen = torch.Generator().manual_seed(77 + N * C * H * W + K)
    bias = torch.randn((K,), generator=gen) * 0.1
    bias[0] = -0.0
    src = torch.randn((N * C * H * W,), generator=gen)
    src[0::7] = 0.0
    src[1::7] = -0.0
    src[2::7] = -1e-40
    src[3::7] = float("nan")
    src[4::7] = -src[4::7].abs() - 1e-30
    assert float(src[2]) < 0 and abs(float(src[2])) < 1.1754944e-38
    return bias, src.view(N, C, H, W)


def accuracy(case, what, got, want64, cpu32, S, Kd, splits, bias=None, relu=False, mask_src=None, extra=0.0):
    """|device - fp64| <= ((Kd + splits + 3) 2^-24 + extra) S[e] + 2^-24 |bias|, per element; torch's float32 CPU result must meet the same
    bound.  Returns the worst device and float32-CPU ratios to the bound."""
    bound = ((Kd + splits + 3) * U + extra) * S
    want, cpu = want64, cpu32
    if bias is not None:
        bb = bias.view(1, -1, 1, 1)
        bound = bound + U * bb.double().abs()
        want, cpu = want + bb.double(), cpu + bb
    if relu:
        want, cpu = want.clamp(min=0), cpu.clamp(min=0)
    if mask_src is not None:
        zero64, zero32 = torch.zeros((), dtype=torch.float64), torch.zeros(())
        want, cpu = torch.where(mask_src > 0, want, zero64), torch.where(mask_src > 0, cpu, zero32)
    got = got.view(want.shape)
    finite = bool(torch.isfinite(got).all())
    tiny = torch.finfo(torch.float64).tiny
    r_dev = float(((got.double() - want).abs() / bound.clamp(min=tiny)).max()) if finite else float("inf")
    r_cpu = float(((cpu.double() - want).abs() / bound.clamp(min=tiny)).max())
    print("MEASURED|%s|%s|%.3f|%.3f" % (case, what, r_dev, r_cpu))
    assert r_cpu <= 1.0, "%s: torch's float32 CPU convolution misses the bound (%.3f of it): the inputs do not suit the rule" % (what, r_cpu)
    assert finite, "%s: non-finite output (an element never written, a read outside an operand, or stale workspace summed)" % what
    assert r_dev <= 1.0, "%s: %.3f of the derived bound (Kd = %d, splits = %d)" % (what, r_dev, Kd, splits)
    return r_dev, r_cpu


def unit_errors(got, want64, S):
    """(max, rms) of |got - fp64| / S over the elements with S > 0."""
    e = (got.double().view(want64.shape) - want64).abs()[S > 0] / S[S > 0]
    return float(e.max()), float((e * e).mean().sqrt())


def check_db(case, db, dy):
    """db within 1 ulp of the float32 rounding of the fp64 sum over images and pixels."""
    want = dy.double().sum((0, 2, 3)).float()
    ulps = ulp_distance(db, want)
    print("MEASURED|%s|db ulp|%d|1" % (case, ulps))
    assert ulps <= 1, "db is %d ulp from the rounded fp64 sum" % ulps


def check_ws(ws, touched, what, finite=True):
    """Exactly the first `touched` floats of the workspace changed, nothing behind them did.  finite: the head holds float32
    slabs, every element written with a finite value; otherwise (packed bf16 pieces, f64 partials) only `no element kept the
    sentinel` is asked."""
    head, rest = ws[:touched], ws[touched:]
    assert rest.numel() >= WS_SLACK and all_bits(rest, WS_BITS), "%s: workspace written behind its first %d floats" % (what, touched)
    if touched and finite:
        assert bool(torch.isfinite(head).all()), "%s: a slab element of the %d promised floats was not written" % (what, touched)
    elif touched:
        assert not bool((head.view(torch.int32) == WS_BITS).any()), "%s: part of the first %d floats was not written" % (what, touched)


def ref_of(kind, ref):
    """(fp64 result, float32 CPU result, |.| product) of an entry point from a ConvRef."""
    return {"fwd": (ref.y64, ref.y32, ref.s_y), "bwd_data": (ref.dx64, ref.dx32, ref.s_dx), "bwd_weight": (ref.dw64, ref.dw32, ref.s_dw)}[kind]


def run_call(call, ins, outs, ws_floats=0, ws_bytes=None, mis=None, mis_by=1, bins=(), bouts=(), bshift=None):
    """One call on a fresh arena.  ins: [(name, tensor or None)], outs: [(name, floats or None)] (None: the pointer is NULL);
    call(ptr, ws_ptr, ws_bytes, stream) -> rc with ptr a dict name -> address (or None).  mis: the name of the one tensor that
    sits mis_by floats past a 16-byte boundary.  Every input is ONE arena item [GUARD NaNs | tensor | GUARD NaNs]: the float in
    front of an operand and the float behind it are NaN.  bins: [(name, uint8 tensor or None)], bouts: [(name, bytes or None)]:
    uint8 operands and outputs (arg-max codes) in a kernel_parity.ByteArena of their own, each at an odd address between at least
    16 sentinel bytes on either side, outputs pre-filled with BYTE_OUT; their addresses join `ptr`, their outputs `out`.  bshift:
    {name: bytes past a 16-byte boundary} for the byte operands that must not sit at the default odd address (0: 16-byte aligned, 2: even).  Returns
    rc, the outputs, the workspace and whether everything else (gaps, guards, inputs, of both arenas) is untouched."""
    assert GUARD % 4 == 0
    guard = bit_pattern(GUARD, GUARD_BITS)
    ar = Arena()
    keys, start, padded = {}, {}, {}
    for name, t in ins:
        if t is not None:
            padded[name] = torch.cat([guard, t.detach().contiguous().reshape(-1).float(), guard])
            keys[name], start[name] = ar.add(padded[name], misaligned=mis_by if mis == name else False), GUARD
    for name, n in outs:
        if n is not None:
            keys[name], start[name] = ar.add(n, misaligned=mis_by if mis == name else False, fill=OUT_BITS), 0
    kws = ar.add(max(ws_floats, 4), fill=WS_BITS)
    ar.upload(dev())
    ptr = {name: (ar.ptr(keys[name]) + 4 * start[name] if name in keys else None) for name, _ in list(ins) + list(outs)}
    bar, bkeys, bgiven = None, {}, {}
    if any(t is not None for _, t in list(bins) + list(bouts)):
        bar = ByteArena()
        for name, t in bins:
            if t is not None:
                bgiven[name] = t.detach().cpu().contiguous().reshape(-1)
                bkeys[name] = bar.add(bgiven[name], shift=(bshift or {}).get(name))
        for name, n in bouts:
            if n is not None:
                bkeys[name] = bar.add(n, fill=BYTE_OUT, shift=(bshift or {}).get(name))
        bar.upload(dev())
    for name, _ in list(bins) + list(bouts):
        assert name not in ptr
        ptr[name] = bar.ptr(bkeys[name]) if name in bkeys else None
    if mis is not None:
        assert ptr[mis] % 16 == 4 * mis_by
    rc = call(ptr, ar.ptr(kws), 4 * ws_floats if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                          # a fault is sticky: end the session instead of launching the remaining cases
        pytest.exit("HIP error after a kernel launch; nothing more is launched: %r" % (e,), returncode=3)
    ar.download()
    r = types.SimpleNamespace(rc=rc, ws=ar.get(kws).clone())
    r.out = {name: ar.get(keys[name]).clone() for name, n in outs if n is not None}
    r.clean = ar.gaps_untouched() and all(bitwise_equal(ar.get(keys[name]), padded[name]) for name in padded)      # guards and inputs
    if bar is not None:
        bar.download()
        r.out.update({name: bar.get(bkeys[name]).clone() for name, n in bouts if n is not None})
        r.clean = r.clean and bar.gaps_untouched() and all(torch.equal(bar.get(bkeys[name]), bgiven[name]) for name in bgiven)
    return r
