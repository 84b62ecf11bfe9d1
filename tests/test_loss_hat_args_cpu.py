"""Argument checks of the entry points of csrc/loss.hip and csrc/hat.hip: every rejection made before a launch returns
CLHIP_EINVAL.  Runs without a GPU: the pointers are dummies that are never dereferenced, because nothing is launched."""
import ctypes as C

EINVAL = -1


def _setup():
    from clsurvey_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    return _lib, L, C.addressof(buf), buf


def test_softmax_ce_slice_rejects_bad_arguments():
    _lib, L, p, _keep = _setup()
    assert L.clhip_softmax_ce_slice(p, p, 4, 8, 5, 4, 0, p, p, None, None) == EINVAL      # col_off + ncols > ld
    assert L.clhip_softmax_ce_slice(p, p, 4, 8, 0, 9, 0, p, p, None, None) == EINVAL
    assert L.clhip_softmax_ce_slice(p, p, 4, 8, 0, 8, 2, p, p, None, None) == EINVAL      # reduction is 0 or 1
    assert L.clhip_softmax_ce_slice(p, p, 4, 8, 0, 8, -1, p, p, None, None) == EINVAL
    assert L.clhip_softmax_ce_slice(p, p, 0, 8, 0, 8, 0, p, p, None, None) == EINVAL      # N <= 0
    assert L.clhip_softmax_ce_slice(p, p, -3, 8, 0, 8, 0, p, p, None, None) == EINVAL
    assert L.clhip_softmax_ce(p, p, 0, 8, 0, p, p, None, None) == EINVAL


def test_lwf_loss_rejects_bad_arguments():
    _lib, L, p, _keep = _setup()

    def call(sizes, N=4, ld=16, ld_t=16, T=2.0, distill=1, teacher=p, n_heads=None):
        hs = (C.c_int * max(len(sizes), 1))(*sizes)
        return L.clhip_lwf_loss(p, p, teacher, hs, len(sizes) if n_heads is None else n_heads, N, ld, ld_t, T, 1.0, distill, p, p, None, None)
    assert call([4, 4], N=1025) == EINVAL                                                  # one thread per row, one block
    assert call([4, 4], N=0) == EINVAL
    assert call([4, 4], T=0.0) == EINVAL
    assert call([4, 4], T=-1.0) == EINVAL
    assert call([], n_heads=0) == EINVAL
    assert call([1] * 33) == EINVAL                                                        # LWF_MAX_HEADS = 32
    assert call([4, 0, 4]) == EINVAL                                                       # an empty head
    assert call([8, 9], ld=16) == EINVAL                                                   # heads wider than ld
    assert call([8, 4], ld=16, ld_t=7) == EINVAL                                           # old heads wider than ld_teacher
    assert call([4, 4], teacher=None) == EINVAL                                            # two heads distilled from no teacher


def test_mse_zero_sum_rejects_an_empty_tensor():
    _lib, L, p, _keep = _setup()
    assert L.clhip_mse_zero_sum(p, 0, p, p, None) == EINVAL


def test_hat_entries_reject_bad_arguments():
    _lib, L, p, _keep = _setup()
    gates = (_lib.HatGateJob * 41)(*[_lib.HatGateJob(p, p, None, 4, 0) for _ in range(41)])
    assert L.clhip_hat_gates_multi(gates, 41, 1.0, p, None) == EINVAL                      # one launch holds 40 jobs
    embs = (_lib.HatEmbJob * 41)(*[_lib.HatEmbJob(p, p, None, p, 4, 2, 0, 0) for _ in range(41)])
    assert L.clhip_hat_emb_grads_multi(embs, 41, 1.0, 0.75, 8.0, p, None) == EINVAL
    assert L.clhip_hat_emb_grads_multi(embs, 1, 1.0, 0.75, 0.0, None, None) == EINVAL      # count = 0 and no sums to read it from
    for n in (1, 45):
        need = L.clhip_hat_sgd_multi_ws(n)
        params = (_lib.HatParam * n)(*[_lib.HatParam(p, p, p, None, 8, 0, 0) for _ in range(n)])
        assert L.clhip_hat_sgd_step_multi(params, n, 0.05, 0.9, 0.0, 0, 1.0, 400.0, 50.0, 1e4, 6.0, 1, p, need - 1, None) == EINVAL
        params[n - 1].n = 0                                                                # an empty parameter, workspace large enough
        assert L.clhip_hat_sgd_step_multi(params, n, 0.05, 0.9, 0.0, 0, 1.0, 400.0, 50.0, 1e4, 6.0, 1, p, need, None) == EINVAL
    for dims in ((0, 3, 9), (7, 0, 9), (7, 3, 0)):
        layers = (_lib.HatLayer * 1)(_lib.HatLayer(p, p, p, *dims))
        assert L.clhip_hat_scale_weights_multi(layers, 1, None) == EINVAL
        jobs = (_lib.HatWgradJob * 1)(_lib.HatWgradJob(p, p, p, p, dims[0], dims[1], dims[2], 0))
        assert L.clhip_hat_weight_grads_multi(jobs, 1, None) == EINVAL
    assert L.clhip_clamp(p, 0, -6.0, 6.0, None) == 0                                       # nothing to do is not an error
