"""The kernel mixture oracle (tests/mixture_oracle.py) against torch.distributions in fp64,
its gradients against torch autograd, and closed-form known answers.  CPU only."""

import numpy as np
import pytest
import torch

import mixture_oracle as MO


def _torch_log_prob(y, t, locs, scales):
    """MixtureSameFamily(Categorical(logits), Independent(Normal(locs, |s|), 1)).log_prob in fp64.
    torch rejects negative scales: passing |s| is what pins the oracle's |s| semantics."""
    D = torch.distributions
    B, M = t.shape
    comp = D.Independent(D.Normal(locs.expand(B, *locs.shape), scales.abs()[None, :, None].expand(B, M, locs.shape[1])), 1)
    return D.MixtureSameFamily(D.Categorical(logits=t), comp).log_prob(y)


@pytest.mark.parametrize("B,M,d", [(7, 1, 1), (5, 6, 3), (9, 100, 1), (4, 65, 2)])
def test_oracle_matches_torch_distributions(B, M, d):
    y, t, locs, s = (np.asarray(a, np.float64) for a in MO.make_inputs(B, M, d))
    ref = _torch_log_prob(*(torch.from_numpy(a) for a in (y, t, locs, s))).numpy()
    got = MO.log_prob(y, t, locs, s)
    assert (s < 0).any() or M == 1  # the default first bandwidth is negative: |s| matters
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    # fused normalisation: log_prob((y - m) / sd) - sum(log sd)
    m, sd = np.linspace(-0.5, 0.5, d), np.linspace(0.5, 2.0, d)
    ref_n = _torch_log_prob(torch.from_numpy((y - m) / sd), *(torch.from_numpy(a) for a in (t, locs, s))).numpy()
    np.testing.assert_allclose(MO.log_prob(y, t, locs, s, m, sd), ref_n - np.log(sd).sum(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,M,d,fused", [(6, 6, 3, False), (5, 100, 1, False), (4, 65, 2, True)])
def test_oracle_gradients_match_autograd(B, M, d, fused):
    y, t, locs, s = (np.asarray(a, np.float64) for a in MO.make_inputs(B, M, d, seed=1))
    g = np.random.default_rng(3).standard_normal(B)
    m, sd = (np.linspace(-0.5, 0.5, d), np.linspace(0.5, 2.0, d)) if fused else (None, None)
    ty, tt, ts = (torch.from_numpy(a).requires_grad_(True) for a in (y, t, s))
    tl = torch.from_numpy(locs)
    yn = (ty - torch.from_numpy(m)) / torch.from_numpy(sd) if fused else ty
    # the oracle's own expression with s (not |s|) outside the log term
    z2 = (((yn[:, None, :] - tl[None]) / ts[None, :, None]) ** 2).sum(-1)
    c = -0.5 * z2 - d * torch.log(ts.abs())[None, :] - 0.5 * d * np.log(2 * np.pi)
    lp = torch.logsumexp(tt + c, -1) - torch.logsumexp(tt, -1)
    (lp * torch.from_numpy(g)).sum().backward()
    gl, gy, gs, gabs = MO.log_prob_grads(y, t, locs, s, g, m, sd)
    np.testing.assert_allclose(gl, tt.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(gy, ty.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(gs, ts.grad.numpy(), rtol=1e-10, atol=1e-11)
    assert (gabs >= np.abs(gs) - 1e-12).all()


def test_single_component_is_the_gaussian_for_any_logit():
    rng = np.random.default_rng(0)
    y = rng.standard_normal((11, 2))
    loc, s = np.array([[0.3, -1.2]]), np.array([-0.3571])
    want = -0.5 * (((y - loc) / s) ** 2).sum(-1) - 2 * np.log(0.3571) - np.log(2 * np.pi)
    for logit in (-50.0, 0.0, 123.0):
        np.testing.assert_allclose(MO.log_prob(y, np.full((11, 1), logit), loc, s), want, rtol=1e-12)


def test_equal_components_give_the_component_density_for_any_logits():
    rng = np.random.default_rng(1)
    y = rng.standard_normal((9, 3))
    locs = np.tile(np.array([[0.5, 0.0, -0.5]]), (7, 1))
    s = np.full((7,), 0.7068)
    want = MO.component_log_prob(y, locs[:1], s[:1])[:, 0]
    np.testing.assert_allclose(MO.log_prob(y, 5 * rng.standard_normal((9, 7)), locs, s), want, rtol=1e-12)


def test_default_scale_vector():
    s = MO.layer_scales(np.zeros(2), (0.3, 0.7), n_centers=3)
    assert s.shape == (6,)
    np.testing.assert_allclose(s, [-0.3571] * 3 + [0.7068] * 3, atol=5e-5)
    np.testing.assert_allclose(MO.half_scales(5), [-0.3571] * 3 + [0.7068] * 2, atol=5e-5)


def test_minus_inf_logit_removes_its_component_and_nonfinite_rows():
    y, t, locs, s = (np.asarray(a, np.float64) for a in MO.make_inputs(4, 6, 1, seed=2))
    t[:, ::2] = -np.inf
    np.testing.assert_allclose(MO.log_prob(y, t, locs, s), MO.log_prob(y, t[:, 1::2], locs[1::2], s[1::2]), rtol=1e-12)
    t[0, :] = -np.inf
    t[1, 1] = np.inf
    t[2, 3] = np.nan
    lp = MO.log_prob(y, t, locs, s)
    assert list(np.isfinite(lp)) == [False, False, False, True]
