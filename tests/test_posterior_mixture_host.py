"""Posterior scores of the two mixture layers, host side: the C ABI's symbols, ctypes
signatures, argument validation and workspace sizes (every call here fails validation or is
a host query, so nothing reaches a GPU), and the estimators' construction."""

import ctypes

import numpy as np
import pytest

from normalizingflownetwork_amd import (BayesianNNEstimator, BayesKernelMixtureNetwork, BayesMixtureDensityNetwork,
                                        BayesNormalizingFlowNetwork, GaussianKernelsLayer, GaussianMixtureLayer,
                                        _lib)

P = 0x1000  # never dereferenced: every call below fails validation

I32, I64, VP = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


def _gmm(lib, y=P, ybs=1, t=P, ds=150, rs=15, S=4, B=10, d=1, K=5, ym=None, ys=None, out=P, osum=None, ws=None):
    return lib.nfn_posterior_lse_gaussian_mixture_f32(y, ybs, t, ds, rs, S, B, d, K, ym, ys, out, osum, ws, None)


def _kern(lib, y=P, ybs=1, t=P, ds=1000, rs=100, S=4, locs=P, scales=P, B=10, d=1, M=100, ym=None, ys=None, out=P,
          osum=None, ws=None):
    return lib.nfn_posterior_lse_kernel_mixture_f32(y, ybs, t, ds, rs, S, locs, scales, B, d, M, ym, ys, out, osum,
                                                    ws, None)


def test_signatures_cover_the_new_symbols(native_lib):
    ws_sig = (I64, [I64, I32, I32])
    want = {
        "nfn_posterior_gaussian_mixture_workspace_doubles": ws_sig,
        "nfn_posterior_kernel_mixture_workspace_doubles": ws_sig,
        "nfn_posterior_lse_gaussian_mixture_f32":
            (I32, [VP, I64, VP, I64, I64, I32, I64, I32, I32, VP, VP, VP, VP, VP, VP]),
        "nfn_posterior_lse_kernel_mixture_f32":
            (I32, [VP, I64, VP, I64, I64, I32, VP, VP, I64, I32, I32, VP, VP, VP, VP, VP, VP]),
    }
    for name, (res, args) in want.items():
        assert name in _lib.SIGNATURES
        assert hasattr(native_lib, name)
        assert _lib.SIGNATURES[name][0] is res, name
        assert list(_lib.SIGNATURES[name][1]) == args, name
    assert native_lib.nfn_version() == 203


@pytest.mark.parametrize("call", [_gmm, _kern])
def test_abi_rejects_bad_draws_and_strides(native_lib, call):
    assert call(native_lib, S=0) == _lib.NFN_E_SHAPE
    assert b"draws" in native_lib.nfn_last_error()
    assert call(native_lib, S=-1) == _lib.NFN_E_SHAPE
    assert call(native_lib, ds=-1) == _lib.NFN_E_SHAPE
    assert b"stride" in native_lib.nfn_last_error()
    assert call(native_lib, rs=-15) == _lib.NFN_E_SHAPE
    assert call(native_lib, ybs=-1) == _lib.NFN_E_SHAPE
    assert call(native_lib, B=-1) == _lib.NFN_E_SHAPE
    assert b"batch" in native_lib.nfn_last_error()
    assert call(native_lib, d=0) == _lib.NFN_E_SHAPE
    assert call(native_lib, d=33, ybs=33, rs=1 << 20) == _lib.NFN_E_SHAPE


def test_abi_rejects_bad_shapes_gmm(native_lib):
    assert _gmm(native_lib, rs=14) == _lib.NFN_E_SHAPE  # row stride < P
    assert b"stride" in native_lib.nfn_last_error()
    assert _gmm(native_lib, K=0) == _lib.NFN_E_SHAPE
    assert _gmm(native_lib, K=342, rs=1026, ds=10260) == _lib.NFN_E_SHAPE  # P = 1026 > 1023
    assert _gmm(native_lib, K=1 << 30, d=32, ybs=32, rs=1 << 40, ds=1 << 44) == _lib.NFN_E_SHAPE
    assert _gmm(native_lib, d=3, K=2, rs=14, ybs=2) == _lib.NFN_E_SHAPE  # y stride < d


def test_abi_rejects_bad_shapes_kernel(native_lib):
    assert _kern(native_lib, rs=99) == _lib.NFN_E_SHAPE  # row stride < M
    assert b"stride" in native_lib.nfn_last_error()
    assert _kern(native_lib, M=0) == _lib.NFN_E_SHAPE
    assert _kern(native_lib, M=1025, rs=1025, ds=10250) == _lib.NFN_E_SHAPE
    assert _kern(native_lib, M=1024, d=32, ybs=32, rs=1024, ds=10240) == _lib.NFN_E_SHAPE  # M * d > 8192


def test_abi_rejects_null_pointers(native_lib):
    for name in ("y", "t"):
        assert _gmm(native_lib, **{name: None}) == _lib.NFN_E_NULLPTR, name
    for name in ("y", "t", "locs", "scales"):
        assert _kern(native_lib, **{name: None}) == _lib.NFN_E_NULLPTR, name
    for call in (_gmm, _kern):
        assert call(native_lib, ym=P, ys=None) == _lib.NFN_E_NULLPTR
        assert call(native_lib, ym=None, ys=P) == _lib.NFN_E_NULLPTR
        assert call(native_lib, osum=P, ws=None) == _lib.NFN_E_NULLPTR  # out_sum needs the workspace


def test_abi_accepts_the_limit_shapes_up_to_the_launch(native_lib):
    """B = 0 passes validation and launches nothing."""
    assert _gmm(native_lib, K=341, d=1, rs=1023, ds=0, B=0) == _lib.NFN_OK  # a draw stride of 0 is a stride
    assert _gmm(native_lib, K=93, d=5, ybs=5, rs=1023, ds=1023, S=1, B=0) == _lib.NFN_OK
    assert _gmm(native_lib, ybs=0, B=0) == _lib.NFN_OK  # a broadcast y row
    assert _kern(native_lib, M=1024, d=8, ybs=8, rs=1024, ds=0, B=0) == _lib.NFN_OK
    assert _kern(native_lib, ybs=0, S=1 << 20, B=0) == _lib.NFN_OK


def test_abi_workspace_sizes_follow_the_single_draw_entries(native_lib):
    for post, single, w in ((native_lib.nfn_posterior_gaussian_mixture_workspace_doubles,
                             native_lib.nfn_gaussian_mixture_workspace_doubles, 5),
                            (native_lib.nfn_posterior_kernel_mixture_workspace_doubles,
                             native_lib.nfn_kernel_mixture_workspace_doubles, 100)):
        sizes = [post(B, 1, w) for B in (1, 2, 63, 64, 65, 4099, 1 << 20, 1 << 22, 1 << 31)]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert sizes == [single(B, 1, w) for B in (1, 2, 63, 64, 65, 4099, 1 << 20, 1 << 22, 1 << 31)]
        assert post(0, 1, w) == 0


def test_estimator_construction_and_defaults():
    m = BayesMixtureDensityNetwork(2, kl_weight_scale=0.1, n_centers=4)
    assert isinstance(m, BayesianNNEstimator) and isinstance(m.dist_layer, GaussianMixtureLayer)
    assert m.dist_layer.n_centers == 4 and m.n_dims == 2
    assert m.hidden_sizes == (10,) and m.activation == "tanh" and m.learning_rate == 3e-2 and not m.map_mode
    k = BayesKernelMixtureNetwork(1, kl_weight_scale=0.1)
    assert isinstance(k, BayesianNNEstimator) and isinstance(k.dist_layer, GaussianKernelsLayer)
    assert k.dist_layer.n_centers == 50 and k.dist_layer.trainable_scale
    assert isinstance(BayesNormalizingFlowNetwork(1), BayesianNNEstimator)
    for cls, layer, n in ((BayesMixtureDensityNetwork, GaussianMixtureLayer, 5),
                          (BayesKernelMixtureNetwork, GaussianKernelsLayer, 50)):
        built = cls.build_function(1, 0.01)
        assert isinstance(built.dist_layer, layer) and built.dist_layer.n_centers == n
        assert built.learning_rate == 2e-2 and built.activation == "tanh" and built.hidden_sizes == (10,)
        assert built.kl_weight_scale == 0.01 and not built.map_mode
    with pytest.raises(AssertionError):
        BayesMixtureDensityNetwork(1, kl_weight_scale=2.0)  # BayesianNNEstimator.py:120
    # the posterior variables: [loc | rho] per layer, loc only in map mode
    m = BayesMixtureDensityNetwork(1, kl_weight_scale=1.0, n_centers=3, hidden_sizes=(4,), n_dims_x=1)
    assert [tuple(w.shape) for w in m._mlp.weights] == [(1, 4), (4, 9)]
    assert len(m.posterior_scales("cpu")) == 2
    mm = BayesMixtureDensityNetwork(1, kl_weight_scale=1.0, n_centers=3, hidden_sizes=(4,), n_dims_x=1,
                                    map_mode=True)
    assert mm.posterior_scales("cpu") is None
    assert np.all(np.isfinite(mm._mlp.weights[0].numpy()))
