"""Numpy oracle of the kernel mixture network's density (``GaussianKernelsLayer``,
estimators/DistributionLayers.py:118-133) and its gradients, parametrised by dtype: run in
float64 it is the reference, in float32 an op-by-op mirror of the same formulas (the naive
``logsumexp(t + c) - logsumexp(t)``, as TF evaluates ``MixtureSameFamily.log_prob``).

    c_bk   = -0.5 * sum_j ((y_bj - locs_kj) / s_k)^2 - d*log|s_k| - 0.5*d*log(2*pi)
    logp_b = logsumexp_k(t_bk + c_bk) - logsumexp_k(t_bk)

``|s|`` enters the log term only: the reference's bandwidths can be negative (include/nfn.h).
"""

import numpy as np

DEFAULT_INIT_SCALES = (0.3, 0.7)


def layer_scales(v, init_scales=DEFAULT_INIT_SCALES, n_centers=1, dtype=np.float64):
    """``softplus(v[i]) + log(expm1(init_scales[i]))`` per scale, each repeated ``n_centers``
    times (DistributionLayers.py:87-97)."""
    v = np.asarray(v, dtype)
    s = np.log1p(np.exp(v)) + np.log(np.expm1(np.asarray(init_scales, dtype)))
    return np.repeat(s.astype(dtype), n_centers)


def half_scales(M, dtype=np.float32):
    """The two default bandwidths (v = 0) by halves of the M components."""
    s = layer_scales(np.zeros(2), dtype=np.float64)
    out = np.where(np.arange(M) < (M + 1) // 2, s[0], s[1])
    return out.astype(dtype)


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


def _r2_z2(y, locs, scales):
    """``r2_bk = sum_j (y_bj - locs_kj)^2`` and ``z2_bk = sum_j ((y_bj - locs_kj) / s_k)^2``, (B, M)."""
    B, M = y.shape[0], locs.shape[0]
    r2 = np.zeros((B, M), y.dtype)
    z2 = np.zeros((B, M), y.dtype)
    for j in range(locs.shape[1]):
        diff = y[:, j, None] - locs[None, :, j]
        r2 += diff * diff
        z = diff / scales[None, :]
        z2 += z * z
    return r2, z2


def component_log_prob(y, locs, scales, dtype=np.float64):
    """``c_bk`` (B, M) for already-normalised ``y`` (B, d)."""
    y = np.asarray(y, dtype)
    locs = np.asarray(locs, dtype)
    scales = np.asarray(scales, dtype)
    d = locs.shape[1]
    _, z2 = _r2_z2(y, locs, scales)
    return dtype(-0.5) * z2 - dtype(d) * np.log(np.abs(scales))[None, :] - dtype(0.5 * d * np.log(2.0 * np.pi))


def log_prob(y, logits, locs, scales, y_mean=None, y_std=None, dtype=np.float64):
    """(B,) log-density; ``y`` (B or 1, d) broadcasts against ``logits`` (B, M)."""
    t = np.asarray(logits, dtype)
    yn, corr = _normalise(y, y_mean, y_std, dtype)
    c = component_log_prob(yn, locs, scales, dtype)
    with np.errstate(all="ignore"):
        return _lse(t + c) - _lse(t) - corr


def log_prob_grads(y, logits, locs, scales, g_out=None, y_mean=None, y_std=None, dtype=np.float64):
    """Gradients of ``L = sum_b g_out[b] * logp_b``: ``(grad_logits (B, M), grad_y (B, d),
    grad_scales (M,), abs_terms (M,))`` where ``abs_terms[k] = sum_b |term_bk|`` over the
    per-sample terms of ``grad_scales`` — what conditions that batch sum."""
    t = np.asarray(logits, dtype)
    locs = np.asarray(locs, dtype)
    scales = np.asarray(scales, dtype)
    B, d = t.shape[0], locs.shape[1]
    g = np.ones((B,), dtype) if g_out is None else np.asarray(g_out, dtype).reshape(-1)
    yn, _ = _normalise(y, y_mean, y_std, dtype)
    yn = np.broadcast_to(yn, (B, d))
    r2, z2 = _r2_z2(yn, locs, scales)
    c = dtype(-0.5) * z2 - dtype(d) * np.log(np.abs(scales))[None, :] - dtype(0.5 * d * np.log(2.0 * np.pi))
    post = _softmax(t + c)
    prior = _softmax(t)
    grad_logits = g[:, None] * (post - prior)
    w = post / (scales * scales)[None, :]
    grad_y = np.empty((B, d), dtype)
    for j in range(d):
        grad_y[:, j] = g * np.sum(w * (locs[None, :, j] - yn[:, j, None]), axis=1)
    if y_std is not None:
        grad_y = grad_y / np.asarray(y_std, dtype)[None, :]
    s3 = scales * scales * scales
    term = g[:, None] * post * (r2 / s3[None, :] - dtype(d) / scales[None, :])
    return grad_logits, grad_y, term.sum(axis=0), np.abs(term).sum(axis=0)


def make_inputs(B, M, d, seed=0, logit_scale=3.0, y_scale=1.0):
    """The GPU tests' inputs: ``y ~ y_scale * N(0,1)``, logits ``logit_scale * N(0,1)``, centres
    uniform in [-2, 2], the default bandwidths by halves (float32 arrays)."""
    rng = np.random.default_rng(1000 * seed + 7 * M + 31 * d + B)
    y = (y_scale * rng.standard_normal((B, d))).astype(np.float32)
    t = (logit_scale * rng.standard_normal((B, M))).astype(np.float32)
    locs = rng.uniform(-2.0, 2.0, (M, d)).astype(np.float32)
    return y, t, locs, half_scales(M)
