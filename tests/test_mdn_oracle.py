"""The mixture density network's numpy oracle (tests/mdn_oracle.py) pinned against
torch.distributions, torch fp64 autograd, a hand-computed case and the reference's row layout."""

import numpy as np
import pytest
import torch

import mdn_oracle as MD

SHAPES = [(1, 1), (2, 1), (5, 1), (5, 3), (7, 4)]


def _torch_log_prob(y, t, K, d):
    """``MixtureSameFamily(Categorical(logits), Independent(Normal(loc, sigma), 1))`` in fp64 on
    slices taken as the reference takes them (DistributionLayers.py:198-212)."""
    comps_loc, comps_sig = [], []
    for start in range(0, 2 * K * d, 2 * d):
        comps_loc.append(t[..., start:start + d])
        comps_sig.append(torch.nn.functional.softplus(0.05 * t[..., start + d:start + 2 * d] + np.log(np.expm1(1.0))))
    loc, sig = torch.stack(comps_loc, dim=1), torch.stack(comps_sig, dim=1)
    logits = t[..., 2 * K * d:2 * K * d + K]
    mix = torch.distributions.MixtureSameFamily(
        torch.distributions.Categorical(logits=logits),
        torch.distributions.Independent(torch.distributions.Normal(loc, sig), 1))
    return mix.log_prob(y)


def test_total_param_size_mixture():
    """tests/test_distribution_layers.py:34-38 (test_total_param_size_mixture)."""
    assert MD.total_param_size(n_dims=5, n_centers=5) == 55
    assert MD.total_param_size(n_dims=1, n_centers=3) == 9


def test_layout_round_trip():
    K, d = 3, 2
    t = np.arange(2 * MD.total_param_size(d, K), dtype=np.float64).reshape(2, -1)
    loc, raw, lg = MD.split(t, K, d)
    np.testing.assert_array_equal(loc[0], [[0, 1], [4, 5], [8, 9]])
    np.testing.assert_array_equal(raw[0], [[2, 3], [6, 7], [10, 11]])
    np.testing.assert_array_equal(lg[0], [12, 13, 14])
    np.testing.assert_array_equal(MD.join(loc, raw, lg), t)
    y, tt = MD.make_inputs(4, K, d)
    assert y.shape == (4, d) and tt.shape == (4, 15) and y.dtype == tt.dtype == np.float32


def test_hand_computed_single_component():
    """K = 1: the logit cancels; raw = 0 gives sigma = softplus(log(expm1(1))) = 1."""
    t = np.array([[0.5, 0.0, 7.0]])
    got = MD.log_prob(np.array([[1.5]]), t, 1, 1)
    assert got[0] == pytest.approx(-0.5 - 0.5 * np.log(2 * np.pi), abs=1e-14)
    # sigma = softplus(0.05 * 20 + log(e - 1)) = log(1 + e (e - 1)), two dims
    s = np.log1p(np.e * (np.e - 1.0))
    t = np.array([[1.0, -1.0, 20.0, 0.0, -3.0]])
    want = -0.5 * ((2.0 - 1.0) / s) ** 2 - np.log(s) - 0.5 * (0.5 + 1.0) ** 2 - np.log(2 * np.pi)
    assert MD.log_prob(np.array([[2.0, 0.5]]), t, 1, 2)[0] == pytest.approx(want, abs=1e-13)
    # with y_mean / y_std: y is normalised and sum(log y_std) subtracted
    got = MD.log_prob(np.array([[3.5]]), np.array([[0.5, 0.0, 7.0]]), 1, 1, np.array([0.5]), np.array([2.0]))
    assert got[0] == pytest.approx(-0.5 - 0.5 * np.log(2 * np.pi) - np.log(2.0), abs=1e-14)


@pytest.mark.parametrize("K,d", SHAPES)
def test_log_prob_matches_torch_distributions(K, d):
    y, t = MD.make_inputs(33, K, d, seed=1)
    want = _torch_log_prob(torch.from_numpy(y.astype(np.float64)), torch.from_numpy(t.astype(np.float64)), K, d).numpy()
    got = MD.log_prob(y, t, K, d)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # y broadcast from one row
    want1 = _torch_log_prob(torch.from_numpy(y[:1].astype(np.float64)), torch.from_numpy(t.astype(np.float64)), K, d)
    np.testing.assert_allclose(MD.log_prob(y[:1], t, K, d), want1.numpy(), rtol=1e-12, atol=1e-12)
    # the float32 mirror is the same function
    got32 = MD.log_prob(y, t, K, d, dtype=np.float32)
    assert got32.dtype == np.float32
    np.testing.assert_allclose(got32, want, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("K,d", SHAPES)
@pytest.mark.parametrize("norm", [False, True])
def test_gradients_match_torch_autograd(K, d, norm):
    B = 17
    y, t = MD.make_inputs(B, K, d, seed=2)
    g = np.random.default_rng(K + d).standard_normal(B)
    ym = np.linspace(-0.5, 0.5, d) if norm else None
    ys = np.linspace(0.5, 2.0, d) if norm else None
    ty = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
    tt = torch.from_numpy(t.astype(np.float64)).requires_grad_(True)
    if norm:
        lp = _torch_log_prob((ty - torch.from_numpy(ym)) / torch.from_numpy(ys), tt, K, d) - float(np.log(ys).sum())
    else:
        lp = _torch_log_prob(ty, tt, K, d)
    np.testing.assert_allclose(MD.log_prob(y, t, K, d, ym, ys), lp.detach().numpy(), rtol=1e-12, atol=1e-12)
    (lp * torch.from_numpy(g)).sum().backward()
    g_t, g_y = MD.log_prob_grads(y, t, K, d, g, ym, ys)
    np.testing.assert_allclose(g_t, tt.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(g_y, ty.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_removed_components_and_nonfinite_rows():
    K, d = 4, 2
    y, t = MD.make_inputs(6, K, d, seed=3)
    t = t.astype(np.float64)
    lg0 = 2 * K * d
    t[:, lg0::2] = -np.inf  # components 0 and 2 removed everywhere
    want = _torch_log_prob(torch.from_numpy(y.astype(np.float64)), torch.from_numpy(t), K, d).numpy()
    np.testing.assert_allclose(MD.log_prob(y, t, K, d), want, rtol=1e-12)
    g_t, g_y = MD.log_prob_grads(y, t, K, d)
    assert np.isfinite(g_t).all() and np.isfinite(g_y).all()
    loc, raw, lg = MD.split(g_t, K, d)
    assert not loc[:, ::2].any() and not raw[:, ::2].any() and not lg[:, ::2].any()
    assert loc[:, 1::2].any()
    t[0, lg0:] = -np.inf
    t[1, lg0 + 1] = np.inf
    t[2, lg0 + 3] = np.nan
    t[3, 1] = np.nan
    assert list(np.flatnonzero(~np.isfinite(MD.log_prob(y, t, K, d)))) == [0, 1, 2, 3]
