"""The posterior-score oracle (tests/posterior_mixture_oracle.py) against torch.logsumexp in
fp64, and its non-finite semantics by hand.  CPU only."""

import numpy as np
import pytest
import torch

import posterior_mixture_oracle as PO


@pytest.mark.parametrize("S,B", [(1, 5), (2, 7), (7, 65), (50, 33)])
def test_posterior_lse_matches_torch_logsumexp(S, B):
    terms = 40.0 * np.random.default_rng(S + B).standard_normal((S, B))
    ref = (torch.logsumexp(torch.from_numpy(terms), dim=0) - np.log(S)).numpy()
    np.testing.assert_allclose(PO.posterior_lse(terms), ref, rtol=1e-14, atol=1e-14)
    got32 = PO.posterior_lse(terms, np.float32)
    assert got32.dtype == np.float32
    np.testing.assert_allclose(got32, ref, rtol=1e-5, atol=1e-5)


def test_single_draw_is_the_term_itself():
    terms = np.array([[-3.5, 0.0, 1e4, -np.inf]])
    np.testing.assert_array_equal(PO.posterior_lse(terms), terms[0])


def test_nonfinite_draws_by_hand():
    inf, nan = np.inf, np.nan
    terms = np.array([
        #  drop   all -inf  NaN    +inf   +inf and -inf   plain
        [-inf, -inf, 1.0, 2.0, inf, 0.0],
        [2.0, -inf, nan, inf, -inf, 0.0],
        [2.0, -inf, 3.0, 0.0, 1.0, 0.0],
    ])
    got = PO.posterior_lse(terms)
    assert got[0] == pytest.approx(2.0 + np.log(2.0) - np.log(3.0), rel=1e-15)  # the -inf draw drops out, S stays 3
    assert got[1] == -inf
    assert np.isnan(got[2])
    assert got[3] == inf
    assert got[4] == inf
    assert got[5] == pytest.approx(0.0, abs=1e-15)


@pytest.mark.parametrize("S", [1, 2, 7])
def test_mixture_posteriors_compose_the_per_draw_oracles(S):
    import mdn_oracle as MD
    import mixture_oracle as MX

    B, K, d = 9, 5, 3
    y, t = PO.make_gmm_inputs(S, B, K, d)
    assert t.shape == (S, B, K * (2 * d + 1)) and t.dtype == np.float32
    np.testing.assert_array_equal(y, MD.make_inputs(B, K, d, seed=3)[0])
    np.testing.assert_array_equal(t[S - 1], MD.make_inputs(B, K, d, seed=100 + S - 1)[1])
    terms = np.stack([MD.log_prob(y, t[s], K, d) for s in range(S)])
    ref = (torch.logsumexp(torch.from_numpy(terms), dim=0) - np.log(S)).numpy()
    np.testing.assert_allclose(PO.gmm_posterior(y, t, K, d), ref, rtol=1e-13, atol=1e-13)
    M = 65
    y, lg, locs, sc = PO.make_kernel_inputs(S, B, M, d)
    assert lg.shape == (S, B, M)
    terms = np.stack([MX.log_prob(y, lg[s], locs, sc) for s in range(S)])
    ref = (torch.logsumexp(torch.from_numpy(terms), dim=0) - np.log(S)).numpy()
    np.testing.assert_allclose(PO.kernel_posterior(y, lg, locs, sc), ref, rtol=1e-13, atol=1e-13)
    ym, ys = np.linspace(-0.5, 0.5, d), np.linspace(0.5, 2.0, d)
    np.testing.assert_allclose(PO.kernel_posterior(y, lg, locs, sc, ym, ys),
                               PO.kernel_posterior((y - ym) / ys, lg, locs, sc) - np.log(ys).sum(),
                               rtol=1e-12, atol=1e-12)
