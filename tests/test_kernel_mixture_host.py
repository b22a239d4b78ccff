"""Kernel mixture network, host side: the layer's bookkeeping and centre selection
(DistributionLayers.py:74-172), the estimator's construction, and the C ABI's argument
validation and workspace sizes (every call here fails validation or is a host query, so
nothing reaches a GPU)."""

import ctypes

import numpy as np
import pytest

from normalizingflownetwork_amd import GaussianKernelsLayer, KernelMixtureNetwork, _lib
from normalizingflownetwork_amd.distribution_layers import cosine_distances, kmeans_centers

import mixture_oracle as MO


def test_total_param_size_and_defaults():
    layer = GaussianKernelsLayer(n_centers=50, n_dims=2)
    assert layer.get_total_param_size() == 100
    assert layer.n_scales == 2 and layer.locs.shape == (100, 2) and not layer.locs.any()
    assert GaussianKernelsLayer(7, 1, init_scales=(0.1, 0.5, 1.0)).get_total_param_size() == 21
    np.testing.assert_allclose(layer.scales().numpy(), MO.layer_scales(np.zeros(2), n_centers=50), atol=1e-6)
    model = KernelMixtureNetwork(1)
    assert model.dist_layer.n_centers == 50 and model.hidden_sizes == (16, 16) and model.learning_rate == 3e-3
    built = KernelMixtureNetwork.build_function()
    assert built.dist_layer.n_centers == 30 and built.learning_rate == 2e-3 and built.activation == "relu"


def test_width_assert_fires_at_call_time():
    layer = GaussianKernelsLayer(n_centers=3, n_dims=1)
    with pytest.raises(AssertionError):
        layer(np.zeros((4, 5), np.float32))


@pytest.mark.parametrize("d", [1, 3])
def test_set_center_points_reference_smallest_case(d):
    """tests/test_ml_estimator.py:19-40: n_centers = 3 on the 10-point ramp — one edge centre
    (the farthest point), two k-means centres among the other nine."""
    y = np.linspace([-1.0] * d, [1.0] * d, 10).reshape((10, d))
    y = (y - y.mean(0)) / y.std(0)
    layer = GaussianKernelsLayer(n_centers=3, n_dims=d)
    layer.set_center_points(y)
    assert layer.locs.shape == (6, d) and layer.locs.dtype == np.float32
    np.testing.assert_array_equal(layer.locs[:3], layer.locs[3:])  # tiled per scale
    far = np.argsort(np.linalg.norm(y - y.mean(0), axis=1))[-2:]
    np.testing.assert_allclose(layer.locs[0], y[far[0]], rtol=1e-6)  # the first of the farthest two
    rest = np.delete(y, far[0], axis=0)
    assert (layer.locs[1:3] >= rest.min() - 1e-6).all() and (layer.locs[1:3] <= rest.max() + 1e-6).all()
    assert not np.allclose(layer.locs[1], layer.locs[2])


def test_set_center_points_shape_tiling_determinism():
    rng = np.random.default_rng(4)
    y = rng.standard_normal((200, 2))
    a, b = GaussianKernelsLayer(10, 2, init_scales=(0.3, 0.7, 1.1)), GaussianKernelsLayer(10, 2, init_scales=(0.3, 0.7, 1.1))
    a.set_center_points(y)
    b.set_center_points(y.copy())
    assert a.locs.shape == (30, 2)
    for i in (1, 2):
        np.testing.assert_array_equal(a.locs[:10], a.locs[10 * i:10 * (i + 1)])
    np.testing.assert_array_equal(a.locs, b.locs)  # one seed, one result
    # n_edge = min(2 d, n_centers // 2) = 4 rim centres are data points among the 8 farthest
    far = set(map(tuple, np.float32(y[np.argsort(np.linalg.norm(y - y.mean(0), axis=1))[-8:]])))
    assert all(tuple(c) in far for c in a.locs[:4])
    assert len({tuple(c) for c in a.locs[:10]}) == 10


def test_kmeans_and_cosine_helpers():
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.normal(-5, 0.1, (30, 2)), rng.normal(5, 0.1, (30, 2))])
    c = kmeans_centers(pts, 2, seed=1)
    assert sorted(np.round(c[:, 0]).tolist()) == [-5.0, 5.0]
    dist = cosine_distances(np.array([[1.0, 0.0], [0.0, 2.0], [-3.0, 0.0]]))
    np.testing.assert_allclose(dist, [[0, 1, 2], [1, 0, 1], [2, 1, 0]], atol=1e-12)


# --- C ABI ----------------------------------------------------------------------------

P = 0x1000  # never dereferenced: every call below fails validation


def _fwd(lib, y=P, ybs=1, logits=P, rs=100, locs=P, scales=P, B=10, d=1, M=100, ym=None, ys=None, out=P, osum=None,
         ws=None):
    return lib.nfn_kernel_mixture_logprob_f32(y, ybs, logits, rs, locs, scales, B, d, M, ym, ys, out, osum, ws, None)


def _grad(lib, y=P, ybs=1, logits=P, rs=100, locs=P, scales=P, B=10, d=1, M=100, gl=P, glrs=100, gy=P, gs=P, ws=P):
    return lib.nfn_kernel_mixture_logprob_grad_f32(y, ybs, logits, rs, locs, scales, B, d, M, None, None, None, None,
                                                   gl, glrs, gy, gs, ws, None)


@pytest.mark.parametrize("call", [_fwd, _grad])
def test_abi_rejects_bad_shapes(native_lib, call):
    for M in (0, 1025):
        assert call(native_lib, M=M, rs=max(M, 1)) == _lib.NFN_E_SHAPE
    assert call(native_lib, d=0) == _lib.NFN_E_SHAPE
    assert call(native_lib, d=33, ybs=33) == _lib.NFN_E_SHAPE
    assert call(native_lib, M=1024, rs=1024, d=9, ybs=9) == _lib.NFN_E_SHAPE  # M * d = 9216 > 8192
    assert call(native_lib, M=100, rs=99) == _lib.NFN_E_SHAPE
    assert call(native_lib, B=-1) == _lib.NFN_E_SHAPE
    assert b"stride" in native_lib.nfn_last_error() or b"batch" in native_lib.nfn_last_error()
    assert _grad(native_lib, glrs=99) == _lib.NFN_E_SHAPE


@pytest.mark.parametrize("call", [_fwd, _grad])
def test_abi_rejects_null_pointers(native_lib, call):
    for name in ("y", "logits", "locs", "scales"):
        assert call(native_lib, **{name: None}) == _lib.NFN_E_NULLPTR, name
    assert _fwd(native_lib, ym=P, ys=None) == _lib.NFN_E_NULLPTR
    assert _fwd(native_lib, osum=P, ws=None) == _lib.NFN_E_NULLPTR  # out_sum needs the workspace
    assert _grad(native_lib, gs=P, ws=None) == _lib.NFN_E_NULLPTR   # grad_scales needs the workspace


def test_abi_workspace_sizes_positive_and_monotone(native_lib):
    for fn in (native_lib.nfn_kernel_mixture_workspace_doubles, native_lib.nfn_kernel_mixture_grad_workspace_floats):
        sizes = [fn(B, 1, 100) for B in (1, 2, 63, 64, 65, 4099, 1 << 20, 1 << 22, 1 << 31)]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert sizes[0] < sizes[-1]
        assert fn(0, 1, 100) == 0
    assert isinstance(native_lib.nfn_kernel_mixture_workspace_doubles, ctypes._CFuncPtr)
