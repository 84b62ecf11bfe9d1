"""Argument checks of the entry points of csrc/pool.hip, csrc/bn.hip, csrc/packnet.hip and csrc/elementwise.hip: every
rejection made before a launch returns CLHIP_EINVAL (CLHIP_ENOSPC for a short BatchNorm workspace), and the n == 0 no-ops
return 0.  Runs without a GPU: the pointers are dummies that are never dereferenced, because nothing is launched."""
import ctypes as C

EINVAL = -1
ENOSPC = -2


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(96)
    p = (C.addressof(buf) + 15) // 16 * 16                  # 16-byte aligned, 80 bytes behind it
    return _lib, L, p, buf


def test_error_codes_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "clhip.h")).read()
    codes = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(CLHIP_E\w+)\s+\(?(-?\d+)\)?", hdr))
    assert codes["CLHIP_EINVAL"] == EINVAL and codes["CLHIP_ENOSPC"] == ENOSPC, codes


def test_maxpool2_rejects_odd_planes_and_float2_misalignment():
    _lib, L, p, _keep = _setup()
    for fn in (L.clhip_maxpool2_fwd, L.clhip_maxpool2_bwd):
        assert fn(p, p, p, 2, 5, 4, None) == EINVAL                                        # odd H
        assert fn(p, p, p, 2, 4, 5, None) == EINVAL                                        # odd W
        assert fn(p, p, p, 0, 4, 4, None) == EINVAL
        assert fn(p, p, p, 2, 0, 4, None) == EINVAL
        assert fn(None, p, p, 2, 4, 4, None) == EINVAL
    # the pointer the kernel reads / writes as float2 must be 8-byte aligned: x of the forward, dx of the backward
    for off in (4, 12):
        assert L.clhip_maxpool2_fwd(p + off, p, p, 2, 4, 4, None) == EINVAL                # (x, y, idx)
        assert L.clhip_maxpool2_bwd(p, p, p + off, 2, 4, 4, None) == EINVAL                # (dy, idx, dx)


def test_maxpool_rejects_bad_windows():
    _lib, L, p, _keep = _setup()
    for fn in (L.clhip_maxpool_fwd, L.clhip_maxpool_bwd):
        assert fn(p, p, p, 2, 8, 8, 0, 1, None) == EINVAL                                  # k = 0
        assert fn(p, p, p, 2, 32, 32, 16, 1, None) == EINVAL                               # k = 16: windows stop at 15 x 15
        assert fn(p, p, p, 2, 8, 8, 3, 0, None) == EINVAL                                  # stride 0
        assert fn(p, p, p, 2, 2, 8, 3, 2, None) == EINVAL                                  # H < k
        assert fn(p, p, p, 2, 8, 2, 3, 2, None) == EINVAL                                  # W < k
        assert fn(p, p, p, 0, 8, 8, 3, 2, None) == EINVAL
        assert fn(p, p, None, 2, 8, 8, 3, 2, None) == EINVAL


def test_batchnorm_rejects_bad_arguments():
    _lib, L, p, _keep = _setup()
    need = L.clhip_bn_ws(3)
    assert need > 0 and L.clhip_bn_ws(0) == 0

    def fwd(N=2, Cc=3, HW=4, training=1, rm=p, rv=p, ws=p, ws_bytes=need, z=p):
        return L.clhip_bn_fwd(z, p, p, rm, rv, p, p, p, N, Cc, HW, training, 0.1, 1e-5, 1, ws, ws_bytes, None)

    def bwd(N=2, Cc=3, HW=4, training=1, relu=1, y=p, ws=p, ws_bytes=need, dz=p):
        return L.clhip_bn_bwd(p, y, p, p, p, p, dz, p, p, N, Cc, HW, training, relu, ws, ws_bytes, None)
    for f in (fwd, bwd):
        assert f(N=0) == EINVAL and f(N=-1) == EINVAL
        assert f(Cc=0) == EINVAL and f(Cc=-2) == EINVAL
        assert f(HW=0) == EINVAL and f(HW=-3) == EINVAL
    assert fwd(z=None) == EINVAL
    assert fwd(training=0, rm=None) == EINVAL                                              # eval mode needs the running statistics
    assert fwd(training=0, rv=None) == EINVAL
    assert fwd(ws_bytes=need - 1) == ENOSPC and fwd(ws=None) == ENOSPC                     # training mode needs the workspace
    assert bwd(relu=1, y=None) == EINVAL                                                   # the ReLU mask is read from y
    assert bwd(dz=None) == EINVAL
    assert bwd(ws_bytes=need - 1) == ENOSPC and bwd(ws=None) == ENOSPC
    assert bwd(training=0, ws_bytes=need - 1) == ENOSPC                                    # the eval backward reduces dgamma / dbeta too


def test_packnet_entries_reject_bad_arguments():
    _lib, L, p, _keep = _setup()
    ws = L.clhip_packnet_kth_ws()
    assert ws >= 261 * 4                                                                   # 260 words and the status word
    assert L.clhip_packnet_kth_abs(p, p, 8, 1, 0, p, p, ws, None) == EINVAL                # k = 0
    assert L.clhip_packnet_kth_abs(p, p, 0, 1, 1, p, p, ws, None) == EINVAL                # n = 0
    assert L.clhip_packnet_kth_abs(p, p, 8, 1, 1 << 32, p, p, ws, None) == EINVAL          # k past 32 bits
    assert L.clhip_packnet_kth_abs(p, p, 8, 1, 1, p, p, ws - 1, None) == EINVAL            # short workspace
    assert L.clhip_packnet_kth_abs(p, p, 8, 1, 1, None, p, ws, None) == EINVAL
    assert L.clhip_packnet_finetune_mask(p, 8, 0, None) == EINVAL                          # 0 is "free", not a task
    assert L.clhip_packnet_finetune_mask(p, 8, 255, None) == EINVAL
    assert L.clhip_packnet_finetune_mask(None, 8, 1, None) == EINVAL
    assert L.clhip_mask_weight_zero(p, p, 8, 2, 1, None) == EINVAL                         # mode is 0 or 1
    assert L.clhip_mask_weight_zero(p, p, 8, -1, 1, None) == EINVAL
    assert L.clhip_packnet_prune(p, p, 8, 1, None, None) == EINVAL                         # no cutoff
    assert L.clhip_mask_grad_zero(p, None, 8, 1, None) == EINVAL
    assert L.clhip_packnet_sgd_step(p, p, None, p, 8, 1, 0.05, 0.9, 5e-4, 1, None) == EINVAL


def test_elementwise_entries_reject_bad_arguments():
    _lib, L, p, _keep = _setup()
    assert L.clhip_fisher_accum(p, p, 8, 0.0, None) == EINVAL                              # data_len <= 0
    assert L.clhip_fisher_accum(p, p, 8, -4.0, None) == EINVAL
    assert L.clhip_mas_accum(p, p, 8, 0.0, 0.0, None) == EINVAL                            # curr_size <= 0
    assert L.clhip_mse_mean(p, p, 0, 1.0, p, p, None) == EINVAL                            # the mean of nothing
    assert L.clhip_mse_mean(p, p, 8, 1.0, p, None, None) == EINVAL
    assert L.clhip_reg_sgd_step(p, p, p, None, p, 8, 400.0, 0.01, 0.9, 0.0, 1, None) == EINVAL     # omega without init_val
    assert L.clhip_si_step(p, p, None, p, p, p, 8, 400.0, 0.01, 0.9, 0.0, 1, None) == EINVAL
    assert L.clhip_si_consolidate(p, p, None, p, 8, 1e-3, None) == EINVAL
    assert L.clhip_relu_bwd(p, None, p, 8, None) == EINVAL
    assert L.clhip_sigmoid_fwd(None, p, 8, None) == EINVAL
    assert L.clhip_sigmoid_bwd(p, None, p, 8, None) == EINVAL
    assert L.clhip_adadelta_step(p, p, None, p, 8, 1.0, 0.9, 1e-6, 0.0, None) == EINVAL
    ptrs = (C.c_void_p * 33)(*([p] * 33))
    assert L.clhip_imm_merge(ptrs, None, None, 0, 8, p, None) == EINVAL                    # 1 .. 32 models
    assert L.clhip_imm_merge(ptrs, None, None, 33, 8, p, None) == EINVAL
    assert L.clhip_imm_merge(ptrs, ptrs, None, 2, 8, p, None) == EINVAL                    # precisions without their sum
    assert L.clhip_imm_merge(ptrs, None, None, 2, 8, None, None) == EINVAL
    holes = (C.c_void_p * 2)(p, None)
    assert L.clhip_imm_merge(holes, None, None, 2, 8, p, None) == EINVAL                   # a missing model


def test_empty_tensors_are_no_ops():
    _lib, L, p, _keep = _setup()
    ptrs = (C.c_void_p * 2)(p, p)
    assert L.clhip_packnet_finetune_mask(p, 0, 1, None) == 0
    assert L.clhip_packnet_prune(p, p, 0, 1, p, None) == 0
    assert L.clhip_mask_grad_zero(p, p, 0, 1, None) == 0
    assert L.clhip_mask_weight_zero(p, p, 0, 1, 1, None) == 0
    assert L.clhip_packnet_sgd_step(p, p, p, None, 0, 1, 0.05, 0.9, 5e-4, 1, None) == 0
    assert L.clhip_reg_sgd_step(p, p, None, None, p, 0, 400.0, 0.01, 0.9, 0.0, 1, None) == 0
    assert L.clhip_fisher_accum(p, p, 0, 8.0, None) == 0
    assert L.clhip_mas_accum(p, p, 0, 0.0, 8.0, None) == 0
    assert L.clhip_si_step(p, p, p, p, p, p, 0, 400.0, 0.01, 0.9, 0.0, 1, None) == 0
    assert L.clhip_si_consolidate(p, p, p, p, 0, 1e-3, None) == 0
    assert L.clhip_relu_bwd(p, p, p, 0, None) == 0
    assert L.clhip_sigmoid_fwd(p, p, 0, None) == 0
    assert L.clhip_sigmoid_bwd(p, p, p, 0, None) == 0
    assert L.clhip_adadelta_step(p, p, p, p, 0, 1.0, 0.9, 1e-6, 0.0, None) == 0
    assert L.clhip_imm_merge(ptrs, None, None, 2, 0, p, None) == 0
