"""Inputs of the sampler's tests, shared by the CPU tests of the oracle
(tests/test_sample_oracle.py, which asserts each regime's defining condition) and the GPU
parity tests (tests/test_gpu_sample.py), and the per-sample backward-error measure both use.

A case is a dict ``ft, d, trainable, eps (B or 1, d), t (B or 1, P), y_mean, y_std`` of
float32 inputs.  The planar regimes place one planar flow of a chain (``stressed``: its
index in ``ft``) where an iterative inverse goes wrong: ``u`` is moved along ``w`` until
``w.u`` hits a drawn target (which fixes ``q = w.u_hat``), then ``b`` is solved from the fp64
oracle so that the root of ``c + q tanh(c + b) = w.z_out`` sits at a drawn ``c + b = delta``.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import nfn_oracle as O

B_REGIME = 4099
C2 = ("planar", "radial") * 5

# regime -> (range of w.u, std of delta = c + b at the root)
PLANAR_REGIMES = {
    "flat": ((-20.0, -8.0), 0.05),        # q -> -1 + 1e-5, root where the slope is ~1.6e-5
    "flat_wide": ((-20.0, -8.0), 2.0),    # the same q over the whole tanh
    "steep": ((2.0, 8.0), 0.3),           # q > 1: Newton oscillates, the bisection fallback runs
    "steep_wide": ((2.0, 8.0), 3.0),
    "saturated": ((-3.0, 3.0), 15.0),     # tanh == +-1 in fp32, dg == 1 exactly
}


def _case(ft, d, trainable, eps, t, y_mean=None, y_std=None, **extra):
    out = dict(ft=tuple(ft), d=d, trainable=trainable, eps=np.ascontiguousarray(eps, np.float32),
               t=np.ascontiguousarray(t, np.float32), y_mean=y_mean, y_std=y_std)
    out.update(extra)
    return out


def random_case(ft, d, B, seed, trainable=True, t_scale=0.5, y_mean=None, y_std=None):
    rng = np.random.default_rng(seed)
    P = O.total_param_size(ft, d, trainable)
    t = (t_scale * rng.standard_normal((B, P))).astype(np.float32)
    eps = rng.standard_normal((B, d)).astype(np.float32)
    return _case(ft, d, trainable, eps, t, y_mean, y_std)


def base_target(case, dt=np.float64):
    """``(target, loc)``: ``loc + scale * eps`` (``eps`` and 0 over a fixed base) in ``dt``."""
    d = case["d"]
    eps = case["eps"].astype(dt)
    if not case["trainable"]:
        return eps, np.zeros((1, d), dt)
    base, _ = O.split_params(case["t"].astype(dt), case["ft"], d, True)
    loc, scale = O.base_params(base, d, True, np.dtype(dt))
    return loc + scale * eps, loc


def planar_regime(regime, ft, d, stressed, seed, B=B_REGIME):
    (lo, hi), dstd = PLANAR_REGIMES[regime]
    assert ft[stressed] == "planar"
    c = random_case(ft, d, B, seed)
    rng = np.random.default_rng(seed + 7919)
    t = c["t"]
    blk = O.split_params(t, ft, d, True)[1][stressed]  # a view: writes land in t
    # keep |w| off 0: reaching w.u there takes a huge u, and the 1e-9 that regularises |w|^2 in
    # _u_circ then lets q fall below -1 (the reference's own constraint fails; no inverse exists)
    blk[(np.square(1.0 + blk[:, d:2 * d].astype(np.float64)).sum(1) < 0.0625), d:2 * d] += np.float32(0.5)
    u, w = blk[:, :d].astype(np.float64), 1.0 + blk[:, d:2 * d].astype(np.float64)
    want = rng.uniform(lo, hi, (B, 1))
    blk[:, :d] = u + (want - (w * u).sum(1, keepdims=True)) * w / (w * w).sum(1, keepdims=True)
    # the flow's input on the inverse walk does not depend on its own b
    t64 = t.astype(np.float64)
    blocks = O.split_params(t64, ft, d, True)[1]
    z_out, _ = base_target(c)
    for k in range(len(ft) - 1, stressed, -1):
        z_out = O.flow_inverse(ft[k], z_out, blocks[k], d)
    u_hat, w, _ = O.planar_params(blocks[stressed], d)
    q = (w * u_hat).sum(1)
    delta = dstd * rng.standard_normal(B)
    blk[:, 2 * d] = delta - ((w * z_out).sum(1) - q * np.tanh(delta))
    c["stressed"] = stressed
    return c


FIXTURE_FT = ("planar", "radial") * 2
FIXTURE_PARTS = (("flat", 0, 86), ("steep", 2, 86), ("saturated", 0, 85))  # regime, stressed flow, rows


def stress_fixture_inputs():
    """``(t, eps)`` of tests/golden/sample_stress_d1.npz (tests/golden/make_golden.py): B = 257
    rows of FIXTURE_FT at d = 1 from the three planar regimes."""
    parts = [planar_regime(r, FIXTURE_FT, 1, k, 700 + i, B=n) for i, (r, k, n) in enumerate(FIXTURE_PARTS)]
    return np.concatenate([p["t"] for p in parts]), np.concatenate([p["eps"] for p in parts])


def planar_stats(case):
    """``(q, c + b)`` of the stressed planar flow at the fp64 oracle's sample."""
    ft, d, k = case["ft"], case["d"], case["stressed"]
    t64 = case["t"].astype(np.float64)
    y, _ = O.chain_sample(case["eps"], t64, ft, d, True)
    blocks = O.split_params(t64, ft, d, True)[1]
    for j in range(k):
        y, _ = O.flow_forward_fldj(ft[j], y, blocks[j], d)
    u_hat, w, b = O.planar_params(blocks[k], d)
    return (w * u_hat).sum(1), (w * y).sum(1) + b[:, 0]


def radial_regime(t0, t1, d, seed, K=1, B=B_REGIME):
    """``K`` radial flows over a fixed base (the target is ``eps`` itself, exactly).  ``t0`` /
    ``t1`` (None = random) set alpha = softplus(0.3 t0 - 2) and beta = softplus(0.1 t1 + c) - 1 of
    every flow: t0 = -40 / +40 gives alpha ~ 8e-7 / ~10, t1 = -60 gives beta ~ -0.996.  Of the last
    flow (the first one inverted): rows 0 mod 3 put the target at
    ``r' = alpha (1 + beta) (1 -+ 1e-3)``, either side of the root formula's branch switch
    (gamma = 0 on half of them, so that fp32 holds the offset); rows 1 mod 3 put it on gamma
    exactly (r' = 0); the rest are random."""
    ft = ("radial",) * K
    c = random_case(ft, d, B, seed, trainable=False)
    rng = np.random.default_rng(seed + 104729)
    t, eps = c["t"], c["eps"]
    for blk in O.split_params(t, ft, d, False)[1]:
        if t0 is not None:
            blk[:, 0] = t0
        if t1 is not None:
            blk[:, 1] = t1
    last = O.split_params(t, ft, d, False)[1][K - 1]
    rows = np.arange(B)
    last[rows % 6 == 0, 2:] = 0.0
    al, be, ga = O.radial_params(last.astype(np.float64), d)
    sw = rows % 3 == 0
    direction = rng.standard_normal((B, d))
    direction /= np.abs(direction).sum(1, keepdims=True)
    rp = al * (1.0 + be) * (1.0 + 1e-3 * np.where((rows // 6) % 2 == 0, 1.0, -1.0))[:, None]
    eps[sw] = (ga + rp * direction)[sw]
    eps[rows % 3 == 1] = last[rows % 3 == 1, 2:]
    c["on_gamma"] = rows % 3 == 1
    c["switch"] = sw
    return c


def radial_branch(case):
    """``A = alpha (1 + beta) - r'`` of the last flow at the fp32 inputs (fp64 arithmetic)."""
    ft, d = case["ft"], case["d"]
    last = O.split_params(case["t"].astype(np.float64), ft, d, False)[1][len(ft) - 1]
    al, be, ga = O.radial_params(last, d)
    return (al * (1.0 + be))[:, 0] - np.abs(case["eps"].astype(np.float64) - ga).sum(1)


def affine_regime(d, seed, B=B_REGIME):
    """One affine flow whose scales 1 + t alternate between 1e-3 and -2."""
    c = random_case(("affine",), d, B, seed)
    blk = O.split_params(c["t"], c["ft"], d, True)[1][0]
    pick = (np.arange(B)[:, None] + np.arange(d)[None, :]) % 2 == 0
    blk[:, d:] = np.where(pick, np.float32(1e-3) - np.float32(1.0), np.float32(-3.0))
    return c


def _regime_cases():
    out = {}
    for i, regime in enumerate(PLANAR_REGIMES):
        for d in (1, 3):
            out[f"planar-{regime}-d{d}"] = functools.partial(planar_regime, regime, ("planar",), d, 0, 300 + 10 * i + d)
    for i, regime in enumerate(("flat", "steep", "saturated")):
        # inside the C2 chain: the stressed planar flow first, in the middle, last
        for k in (0, 4, 8):
            out[f"c2-{regime}-at{k}"] = functools.partial(planar_regime, regime, C2, 1, k, 400 + 10 * i + k)
    for i, (t0, t1) in enumerate(((-40.0, None), (40.0, None), (None, -60.0), (-40.0, -60.0), (40.0, -60.0))):
        for d in (1, 3):
            out[f"radial-t0={t0}-t1={t1}-d{d}"] = functools.partial(radial_regime, t0, t1, d, 500 + 10 * i + d)
    out["radial3-t0=-40-t1=-60-d1"] = functools.partial(radial_regime, -40.0, -60.0, 1, 560, K=3)
    out["radial3-t0=40-t1=-60-d1"] = functools.partial(radial_regime, 40.0, -60.0, 1, 561, K=3)
    for d in (1, 3):
        out[f"affine-scales-d{d}"] = functools.partial(affine_regime, d, 600 + d)
    return out


REGIME_CASES = _regime_cases()


@functools.lru_cache(maxsize=None)
def regime_case(name):
    return REGIME_CASES[name]()


# ---- the shape and path matrix ----------------------------------------------------------------------

SMALL_B = (1, 63, 64, 65, 255, 256, 257)
NORM = dict(y_mean=np.array([0.3, -1.0, 2.0], np.float32), y_std=np.array([0.5, 1.25, 2.0], np.float32))
# name -> (flows, d, B, tile rows of the chain's P, random_case keywords); B is ragged against the tile
SHAPES = {f"a-{n}-B{B}": (ft, d, B, 256, {}) for n, ft, d in (("c2", C2, 1), ("rr", ("radial", "radial"), 1),
                                                              ("p6", ("planar",) * 6, 2)) for B in SMALL_B}
SHAPES.update({
    "b-d5-dm8": (("planar", "radial", "planar"), 5, 2 * 256 + 3, 256, {}),
    "c-d16": (("planar", "radial", "affine"), 16, 4 * 64 + 1, 64, {}),
    "d-d17-dm32": (("radial", "planar"), 17, 2 * 128 + 1, 128, {}),
    "e-d32-p10": (("planar",) * 10, 32, 32 * 3 + 5, 32, {}),
    "f-d32-p64": (("planar",) * 64, 32, 67, 8, {}),
    "g-r16": (("radial",) * 16, 1, 2 * 192 + 1, 192, {}),
    "h-r22": (("radial",) * 22, 1, 2 * 128 + 1, 128, {}),
    "i-normalised": (("affine", "planar", "radial"), 3, 2 * 256 + 1, 256, NORM),
    "j-fixed-base": (("affine", "planar", "radial"), 3, 2 * 256 + 1, 256, dict(trainable=False)),
    "k-no-flows-fixed-base": ((), 2, 300, 256, dict(trainable=False)),
    "k-no-flows": ((), 2, 300, 256, {}),
})
EXPECT_P = {"c-d16": 115, "e-d32-p10": 714, "f-d32-p64": 4224, "g-r16": 50, "h-r22": 68, "i-normalised": 24,
            "k-no-flows-fixed-base": 0}


def tile_rows(P):
    """tile_geom of nfn_api.hip: 256 rows while the tile (odd row stride P | 1) fits 48 KiB,
    else fewer by 64 down to 64, then halved until it fits the 156 KiB a workgroup may take."""
    row = (P | 1) * 4
    rows = 256
    while rows > 64 and rows * row > 48 * 1024:
        rows -= 64
    while rows > 1 and rows * row > 156 * 1024:
        rows >>= 1
    return rows


# ---- the backward error of a sample ---------------------------------------------------


def backward_error(case, y):
    """``(z_K, target, err, unit)`` of samples ``y`` (B, d): the fp64 forward chain of
    ``z_0 = y`` (``(y - y_mean) / y_std`` when the case normalises) against
    ``target = loc + scale eps``, ``err = |z_K - target|_inf``, in units of

        unit = 2^-24 sum_{k=0..K} |M_k|_inf s_k,    M_k = J_{K-1} ... J_k,  M_K = I,

    one half-ulp rounding of each ``z_k`` (and of the flow's additive parameter: ``u_hat``,
    ``gamma`` or ``shift``) carried to the end of the chain by the Jacobians of the flows after
    it: ``s_k = max(1, |z_k|, |z_{k+1}|, |param_k|)``, ``s_K = max(1, |target|, |loc|)`` (max norms)."""
    ft, d = case["ft"], case["d"]
    t64 = case["t"].astype(np.float64)
    target, loc = base_target(case)
    z = np.asarray(y, np.float64)
    if case["y_mean"] is not None:
        z = (z - case["y_mean"].astype(np.float64)) / case["y_std"].astype(np.float64)
    B = z.shape[0]
    blocks = O.split_params(t64, ft, d, case["trainable"])[1]
    amax = lambda a: np.broadcast_to(np.abs(a).max(-1), (B,))  # noqa: E731
    jac, scale = [], []
    with np.errstate(all="ignore"):
        for f, tk in zip(ft, blocks):
            jac.append(O.flow_jacobian(f, z, tk, d))
            par = {"planar": lambda: O.planar_params(tk, d)[0], "radial": lambda: O.radial_params(tk, d)[2],
                   "affine": lambda: O.affine_params(tk, d)[0]}[f]()
            z_next, _ = O.flow_forward_fldj(f, z, tk, d)
            scale.append(np.maximum.reduce([np.ones(B), amax(z), amax(z_next), amax(par)]))
            z = z_next
        M = np.broadcast_to(np.eye(d), (B, d, d))
        unit = np.maximum.reduce([np.ones(B), amax(target), amax(loc)])
        for k in range(len(ft) - 1, -1, -1):
            M = M @ jac[k]
            unit = unit + np.abs(M).sum(-1).max(-1) * scale[k]
        err = np.abs(z - target).max(-1)
    return z, np.broadcast_to(target, z.shape), err, 2.0 ** -24 * unit


@functools.lru_cache(maxsize=None)
def _reference_ratio(key):
    case = _KEYED[key]
    with np.errstate(all="ignore"):
        y32, _ = O.chain_sample(case["eps"], case["t"], case["ft"], case["d"], case["trainable"], case["y_mean"],
                                case["y_std"], np.float32)
    _, _, err, unit = backward_error(case, y32)
    fin = np.isfinite(err) & np.isfinite(unit)
    return float((err[fin] / unit[fin]).max()) if fin.any() else 0.0


_KEYED = {}


def reference_ratio(key, case):
    """``R_ref``: the largest ``err / unit`` of the oracle's own op-by-op fp32 sampler on the case
    (computed once per ``key``: the math modes share it)."""
    _KEYED.setdefault(key, case)
    return _reference_ratio(key)
