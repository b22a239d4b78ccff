"""Host side of the estimators' training step (no GPU): the two "what a step trains" objects on
CPU tensors, and the one path from ``x`` to the normalised network input."""

import numpy as np
import pytest
import torch

from normalizingflownetwork_amd import BayesNormalizingFlowNetwork, NormalizingFlowNetwork
from normalizingflownetwork_amd.estimators import _MeanFieldWeights, _PointWeights

CPU = torch.device("cpu")


def _state(m):
    out = [t.clone() for t in m._mlp.weights + m._mlp.biases]
    if getattr(m, "_post_rho", None) is not None:
        out += [t.clone() for pair in m._post_rho for t in pair]
    return out


def test_point_weights_report_and_write_back():
    m = NormalizingFlowNetwork(1, n_flows=2, hidden_sizes=(4,), n_dims_x=1)
    before = _state(m)
    trained = m._trainables(CPU)
    assert isinstance(trained, _PointWeights)
    assert len(trained.parameters) == 4 and trained.draw_size is None  # two kernels, two biases
    assert all(p.requires_grad and p.is_leaf for p in trained.parameters)
    net, penalty = trained.network(None)
    assert net is m._mlp and penalty is None and net.weights[0] is trained.parameters[0]
    trained.finish()
    after = _state(m)
    assert not any(t.requires_grad for t in m._mlp.weights + m._mlp.biases)
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(after, before))


@pytest.mark.parametrize("map_mode,trainable_prior,n_params", [(False, False, 2), (False, True, 3), (True, False, 1)])
def test_mean_field_weights_report_and_write_back(map_mode, trainable_prior, n_params):
    m = BayesNormalizingFlowNetwork(1, kl_weight_scale=0.5, n_flows=2, hidden_sizes=(4,), n_dims_x=1,
                                    map_mode=map_mode, trainable_prior=trainable_prior)
    point = m._trainables(CPU)  # the default fit trains the means
    assert isinstance(point, _PointWeights)
    point.finish()
    before, N = _state(m), sum(m._layer_sizes())
    trained = m._trainables(CPU, variational=True)
    assert isinstance(trained, _MeanFieldWeights)
    assert len(trained.parameters) == n_params and all(p.numel() == N and p.requires_grad for p in trained.parameters)
    assert trained.draw_size == (0 if map_mode else N)
    trained.finish()
    after = _state(m)
    assert len(after) == len(before) and all(torch.equal(a, b) and a.shape == b.shape for a, b in zip(after, before))
    assert (m._post_rho is None) == map_mode
    assert m._prior_loc.shape == (N,) and not m._prior_loc.any() and not m._prior_loc.requires_grad


def test_normalised_x_is_one_path(monkeypatch):
    rng = np.random.default_rng(4)
    x = rng.standard_normal(7).astype(np.float32)
    m = NormalizingFlowNetwork(1, n_flows=2, hidden_sizes=(4,))
    m.set_data_normalization(x[:, None], x[:, None])
    builds = []
    build = m._build
    monkeypatch.setattr(m, "_build", lambda n: (builds.append(n), build(n)))
    assert m._mlp is None
    flat = m._normalised_x(x, CPU)
    mlp = m._mlp
    column = m._normalised_x(x[:, None], CPU)
    assert builds == [1] and m._mlp is mlp  # built lazily, exactly once
    assert flat.shape == (7, 1) and torch.equal(flat, column)
    want = (x[:, None] - m.x_mean) / (m.x_std + np.float32(1e-8))
    np.testing.assert_array_equal(flat.numpy(), want.astype(np.float32))
