"""Numpy oracle of the mixture density network's density (``GaussianMixtureLayer``,
estimators/DistributionLayers.py:174-212) and its gradients, parametrised by dtype: run in
float64 it is the reference, in float32 an op-by-op mirror of the same formulas in the naive
order ``logsumexp(l - logsumexp(l) + c)``, as TF evaluates ``Mixture.log_prob``.

Row layout (``P = K (2 d + 1)``): ``[loc_0 (d) | raw_0 (d) | ... | loc_{K-1} | raw_{K-1} | logits (K)]``.

    sigma_kj = softplus(0.05 * raw_kj + log(expm1(1)))
    z_kj     = (y_j - loc_kj) / sigma_kj
    c_k      = -0.5 * sum_j z_kj^2 - sum_j log sigma_kj - 0.5 * d * log(2 pi)
    logp     = logsumexp_k(l_k + c_k) - logsumexp_k(l_k)   [- sum_j log y_std_j]
"""

import numpy as np

LOG_EXPM1_ONE = float(np.log(np.expm1(1.0)))


def total_param_size(n_dims, n_centers):
    """``GaussianMixtureLayer.get_total_param_size`` (DistributionLayers.py:188-194)."""
    return n_centers + 2 * n_dims * n_centers


def split(t, K, d, dtype=np.float64):
    """``(loc (B, K, d), raw (B, K, d), logits (B, K))`` of rows ``t`` (B, P)."""
    t = np.asarray(t, dtype)
    assert t.shape[-1] == total_param_size(d, K)
    blocks = t[:, :2 * K * d].reshape(t.shape[0], K, 2, d)
    return blocks[:, :, 0, :], blocks[:, :, 1, :], t[:, 2 * K * d:]


def join(loc, raw, logits):
    """The inverse of :func:`split`."""
    B, K, d = loc.shape
    blocks = np.stack([loc, raw], axis=2).reshape(B, 2 * K * d)
    return np.concatenate([blocks, logits], axis=1)


def _lse(a):
    """tf.reduce_logsumexp over the last axis: the maximum is subtracted where it is finite."""
    with np.errstate(all="ignore"):
        m = np.max(a, axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0).astype(a.dtype)
        return (np.log(np.sum(np.exp(a - m), axis=-1, keepdims=True)) + m)[..., 0]


def _softmax(a):
    with np.errstate(all="ignore"):
        m = np.max(a, axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0).astype(a.dtype)
        e = np.exp(a - m)
        return e / np.sum(e, axis=-1, keepdims=True)


def _normalise(y, y_mean, y_std, dtype):
    y = np.asarray(y, dtype)
    if y_mean is None:
        return y, dtype(0.0)
    ys = np.asarray(y_std, dtype)
    return (y - np.asarray(y_mean, dtype)) / ys, np.sum(np.log(ys)).astype(dtype)


def _parts(yn, t, K, d, dtype):
    """``x, sigma, z`` (B, K, d), ``c`` (B, K) and the logits for already-normalised ``yn``."""
    loc, raw, lg = split(t, K, d, dtype)
    with np.errstate(all="ignore"):
        x = dtype(0.05) * raw + dtype(LOG_EXPM1_ONE)
        sigma = np.logaddexp(dtype(0.0), x).astype(dtype)  # softplus
        z = (yn[:, None, :] - loc) / sigma
        c = dtype(-0.5) * np.sum(z * z, axis=-1) - np.sum(np.log(sigma), axis=-1) - dtype(0.5 * d * np.log(2.0 * np.pi))
    return x, sigma, z, c, lg


def log_prob(y, t, K, d, y_mean=None, y_std=None, dtype=np.float64):
    """(B,) log-density; ``y`` (B or 1, d) broadcasts against ``t`` (B, P)."""
    yn, corr = _normalise(y, y_mean, y_std, dtype)
    B = np.asarray(t).shape[0]
    yn = np.broadcast_to(yn, (B, d))
    _, _, _, c, lg = _parts(yn, t, K, d, dtype)
    with np.errstate(all="ignore"):
        return _lse(lg - _lse(lg)[:, None] + c) - corr


def log_prob_grads(y, t, K, d, g_out=None, y_mean=None, y_std=None, dtype=np.float64):
    """Gradients of ``L = sum_b g_out[b] * logp_b``: ``(grad_t (B, P) in t's layout, grad_y (B, d))``."""
    B = np.asarray(t).shape[0]
    g = np.ones((B,), dtype) if g_out is None else np.asarray(g_out, dtype).reshape(-1)
    yn, _ = _normalise(y, y_mean, y_std, dtype)
    yn = np.broadcast_to(yn, (B, d))
    x, sigma, z, c, lg = _parts(yn, t, K, d, dtype)
    with np.errstate(all="ignore"):
        post = _softmax(lg + c)
        prior = _softmax(lg)
        g_lg = g[:, None] * (post - prior)
        gp = (g[:, None] * post)[:, :, None]
        sig = dtype(1.0) / (dtype(1.0) + np.exp(-x))
        live = gp != 0  # a removed component contributes exact zeros
        g_loc = np.where(live, gp * z / sigma, dtype(0.0))
        g_raw = np.where(live, gp * (z * z - dtype(1.0)) / sigma * dtype(0.05) * sig, dtype(0.0))
        g_y = -np.sum(g_loc, axis=1)
    if y_std is not None:
        g_y = g_y / np.asarray(y_std, dtype)[None, :]
    return join(g_loc, g_raw, g_lg).astype(dtype), g_y.astype(dtype)


def make_inputs(B, K, d, seed=0, loc_scale=2.0, raw_scale=10.0, logit_scale=3.0, y_scale=1.0):
    """The GPU tests' inputs in the reference's interleaved row layout (float32 arrays):
    ``y ~ y_scale * N(0,1)``, locations uniform in ``[-loc_scale, loc_scale]``, raw scales
    ``raw_scale * N(0,1)``, logits ``logit_scale * N(0,1)``.  Returns ``(y (B, d), t (B, P))``."""
    rng = np.random.default_rng(1000 * seed + 7 * K + 31 * d + B)
    y = (y_scale * rng.standard_normal((B, d))).astype(np.float32)
    loc = rng.uniform(-loc_scale, loc_scale, (B, K, d))
    raw = raw_scale * rng.standard_normal((B, K, d))
    lg = logit_scale * rng.standard_normal((B, K))
    return y, join(loc, raw, lg).astype(np.float32)
