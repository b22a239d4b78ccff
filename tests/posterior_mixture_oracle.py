"""Numpy oracle of the Bayesian mixture estimators' posterior score
(``BayesianNNEstimator.score``, estimators/BayesianNNEstimator.py:65-76):

    out_b = logsumexp_s(logp(y_b | row(s, b))) - log S

with ``tf.reduce_logsumexp`` semantics over the draws (axis 0): the maximum is subtracted
only where it is finite, so a ``-inf`` draw drops out, all ``-inf`` gives ``-inf``, a NaN
draw gives NaN and a ``+inf`` draw ``+inf``.  The per-draw terms are ``mdn_oracle.log_prob`` /
``mixture_oracle.log_prob``.  Parametrised by dtype like those: float64 is the reference,
float32 the op-by-op mirror.

Inputs of a case: ``y`` (and the kernel mixture's ``locs`` / ``scales``) come from
``make_inputs(..., seed=3)``, draw ``s``'s rows from ``make_inputs(..., seed=100 + s)``.
"""

import numpy as np

import mdn_oracle as MD
import mixture_oracle as MX


def posterior_lse(terms, dtype=np.float64):
    """``logsumexp`` over axis 0 of ``terms`` (S, B) minus ``log S``: (B,)."""
    a = np.asarray(terms, dtype)
    with np.errstate(all="ignore"):
        m = np.max(a, axis=0, keepdims=True)
        m = np.where(np.isfinite(m), m, 0).astype(dtype)
        lse = (np.log(np.sum(np.exp(a - m), axis=0, keepdims=True)) + m)[0]
        return (lse - np.log(dtype(a.shape[0]))).astype(dtype)


def gmm_terms(y, t_draws, K, d, y_mean=None, y_std=None, dtype=np.float64):
    """(S, B) per-draw log-densities of the Gaussian mixture; ``t_draws`` (S, B, P)."""
    return np.stack([MD.log_prob(y, t, K, d, y_mean, y_std, dtype) for t in t_draws])


def gmm_posterior(y, t_draws, K, d, y_mean=None, y_std=None, dtype=np.float64):
    return posterior_lse(gmm_terms(y, t_draws, K, d, y_mean, y_std, dtype), dtype)


def kernel_terms(y, logits_draws, locs, scales, y_mean=None, y_std=None, dtype=np.float64):
    """(S, B) per-draw log-densities of the kernel mixture; ``logits_draws`` (S, B, M)."""
    return np.stack([MX.log_prob(y, t, locs, scales, y_mean, y_std, dtype) for t in logits_draws])


def kernel_posterior(y, logits_draws, locs, scales, y_mean=None, y_std=None, dtype=np.float64):
    return posterior_lse(kernel_terms(y, logits_draws, locs, scales, y_mean, y_std, dtype), dtype)


def make_gmm_inputs(S, B, K, d, **scaling):
    """``(y (B, d), t_draws (S, B, P))``, float32."""
    y = MD.make_inputs(B, K, d, seed=3, **scaling)[0]
    return y, np.stack([MD.make_inputs(B, K, d, seed=100 + s, **scaling)[1] for s in range(S)])


def make_kernel_inputs(S, B, M, d, **scaling):
    """``(y (B, d), logits_draws (S, B, M), locs (M, d), scales (M,))``, float32."""
    y, _, locs, scales = MX.make_inputs(B, M, d, seed=3, **scaling)
    return y, np.stack([MX.make_inputs(B, M, d, seed=100 + s, **scaling)[1] for s in range(S)]), locs, scales
