"""Mixture density network, host side: the layer's and the distribution's shapes
(tests/test_distribution_layers.py:34-62 of the reference), the estimator's construction, and
the C ABI's argument validation and workspace sizes (every call here fails validation or is a
host query, so nothing reaches a GPU)."""

import numpy as np
import pytest

from normalizingflownetwork_amd import (GaussianMixtureDistribution, GaussianMixtureLayer, MixtureDensityNetwork,
                                        _lib)

import mdn_oracle as MD


def test_total_param_size_mixture():
    assert GaussianMixtureLayer(n_dims=5, n_centers=5).get_total_param_size() == 55
    assert GaussianMixtureLayer(n_dims=1, n_centers=3).get_total_param_size() == 9
    for d, K in ((5, 5), (1, 3), (32, 15)):
        assert GaussianMixtureLayer(n_dims=d, n_centers=K).get_total_param_size() == MD.total_param_size(d, K)


def test_mixture_dist_fn():
    layer = GaussianMixtureLayer(n_dims=1, n_centers=5)
    for B in (1, 3):
        dist = layer(np.ones((B, 15), np.float32))
        assert isinstance(dist, GaussianMixtureDistribution)
        assert dist.event_shape == [1]
        assert dist.batch_shape == [B]
    with pytest.raises(AssertionError):
        layer(np.ones((10, 10), np.float32))
    layer = GaussianMixtureLayer(n_dims=3, n_centers=5)
    for B in (1, 3):
        dist = layer(np.ones((B, 35), np.float32))
        assert dist.event_shape == [3]
        assert dist.batch_shape == [B]
    with pytest.raises(AssertionError):
        layer(np.ones((3, 15), np.float32))


def test_layer_hooks_and_estimator_defaults():
    layer = GaussianMixtureLayer(n_centers=5, n_dims=2)
    assert layer.trainable_parameters("cpu") == []
    assert layer.finish_training() is None
    model = MixtureDensityNetwork(2, n_centers=4)
    assert isinstance(model.dist_layer, GaussianMixtureLayer)
    assert model.dist_layer.n_centers == 4 and model.n_dims == 2
    assert model.hidden_sizes == (16, 16) and model.learning_rate == 3e-3
    assert model._fused_dense_inputs(np.zeros((1, 2), np.float32)) is None  # no flow chain to fuse the Dense layer into
    built = MixtureDensityNetwork.build_function()
    assert built.dist_layer.n_centers == 5 and built.n_dims == 1
    assert built.learning_rate == 2e-3 and built.activation == "relu" and built.hidden_sizes == (16, 16)


# --- C ABI ----------------------------------------------------------------------------

P = 0x1000  # never dereferenced: every call below fails validation


def _fwd(lib, y=P, ybs=1, t=P, rs=15, B=10, d=1, K=5, ym=None, ys=None, out=P, osum=None, ws=None):
    return lib.nfn_gaussian_mixture_logprob_f32(y, ybs, t, rs, B, d, K, ym, ys, out, osum, ws, None)


def _grad(lib, y=P, ybs=1, t=P, rs=15, B=10, d=1, K=5, ym=None, ys=None, gt=P, gtrs=15, gy=P):
    return lib.nfn_gaussian_mixture_logprob_grad_f32(y, ybs, t, rs, B, d, K, ym, ys, None, None, gt, gtrs, gy, None)


def test_signatures_cover_the_new_symbols(native_lib):
    for name in ("nfn_gaussian_mixture_workspace_doubles", "nfn_gaussian_mixture_logprob_f32",
                 "nfn_gaussian_mixture_logprob_grad_f32"):
        assert name in _lib.SIGNATURES
        assert hasattr(native_lib, name)
    assert len(_lib.SIGNATURES["nfn_gaussian_mixture_logprob_f32"][1]) == 13
    assert len(_lib.SIGNATURES["nfn_gaussian_mixture_logprob_grad_f32"][1]) == 15
    assert native_lib.nfn_version() == 203


@pytest.mark.parametrize("call", [_fwd, _grad])
def test_abi_rejects_bad_shapes(native_lib, call):
    assert call(native_lib, K=0) == _lib.NFN_E_SHAPE
    assert call(native_lib, K=-3) == _lib.NFN_E_SHAPE
    assert call(native_lib, d=0) == _lib.NFN_E_SHAPE
    assert call(native_lib, d=33, ybs=33, rs=5 * 67) == _lib.NFN_E_SHAPE
    assert call(native_lib, K=342, rs=1026) == _lib.NFN_E_SHAPE        # P = 1026 > 1023
    assert call(native_lib, K=16, d=32, ybs=32, rs=1040) == _lib.NFN_E_SHAPE  # P = 1040
    assert call(native_lib, K=1 << 30, d=32, ybs=32, rs=1 << 40) == _lib.NFN_E_SHAPE  # no 32-bit wrap of P
    assert call(native_lib, rs=14) == _lib.NFN_E_SHAPE
    assert b"stride" in native_lib.nfn_last_error()
    assert call(native_lib, B=-1) == _lib.NFN_E_SHAPE
    assert b"batch" in native_lib.nfn_last_error()
    assert call(native_lib, ybs=-1) == _lib.NFN_E_SHAPE
    assert call(native_lib, d=3, K=2, rs=14, ybs=2) == _lib.NFN_E_SHAPE  # y stride < d
    assert _grad(native_lib, gtrs=14) == _lib.NFN_E_SHAPE


@pytest.mark.parametrize("call", [_fwd, _grad])
def test_abi_rejects_null_pointers(native_lib, call):
    for name in ("y", "t"):
        assert call(native_lib, **{name: None}) == _lib.NFN_E_NULLPTR, name
    assert call(native_lib, ym=P, ys=None) == _lib.NFN_E_NULLPTR
    assert call(native_lib, ym=None, ys=P) == _lib.NFN_E_NULLPTR
    assert _fwd(native_lib, osum=P, ws=None) == _lib.NFN_E_NULLPTR  # out_sum needs the workspace


def test_abi_accepts_the_limit_shapes_up_to_the_launch(native_lib):
    """B = 0 passes validation and launches nothing: the widest rows are accepted."""
    assert _fwd(native_lib, K=93, d=5, ybs=5, rs=1023, B=0) == _lib.NFN_OK
    assert _fwd(native_lib, K=341, d=1, rs=1023, B=0) == _lib.NFN_OK
    assert _grad(native_lib, K=15, d=32, ybs=32, rs=975, gtrs=975, B=0) == _lib.NFN_OK
    assert _fwd(native_lib, y=P, ybs=0, B=0) == _lib.NFN_OK  # a broadcast y row


def test_abi_workspace_sizes_positive_and_monotone(native_lib):
    fn = native_lib.nfn_gaussian_mixture_workspace_doubles
    sizes = [fn(B, 1, 5) for B in (1, 2, 63, 64, 65, 4099, 1 << 20, 1 << 22, 1 << 31)]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] < sizes[-1]
    assert fn(0, 1, 5) == 0
