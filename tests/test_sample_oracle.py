"""Pins the oracle's inverse side (``flow_inverse``, ``chain_sample``, ``flow_jacobian``)
before the GPU tests trust it as the sampler's checker, and asserts that the generated
regimes of tests/sample_cases.py are the regimes they claim to be (no device needed).

The reference cannot sample (its flows define no inverse), so nothing here restates it:
the inverse is pinned by the forward maps it inverts (fp64 round trip), the Jacobians by
torch autodiff of the independent forward restatement of tests/test_oracle.py, plus analytic
known answers and a committed fixture."""

import math

import numpy as np
import pytest
import torch

import sample_cases as S
from conftest import load_golden
from oracle import nfn_oracle as O
from test_oracle import F64, T_FWD

REGIMES = sorted(S.REGIME_CASES)


def _walk_round_trip(case):
    """Largest per-sample |forward(inverse(z_out)) - z_out|_inf / max(1, |z_out|_inf) over the
    flows of the chain's inverse walk."""
    ft, d = case["ft"], case["d"]
    blocks = O.split_params(case["t"].astype(np.float64), ft, d, case["trainable"])[1]
    z_out, _ = S.base_target(case)
    z_out = np.broadcast_to(z_out, (max(z_out.shape[0], case["t"].shape[0]), d))
    worst = 0.0
    for k in range(len(ft) - 1, -1, -1):
        z = O.flow_inverse(ft[k], z_out, blocks[k], d)
        back, _ = O.flow_forward_fldj(ft[k], z, blocks[k], d)
        rel = np.abs(back - z_out).max(1) / np.maximum(1.0, np.abs(z_out).max(1))
        assert np.isfinite(rel).all(), (ft[k], k)
        worst = max(worst, float(rel.max()))
        z_out = z
    return worst


@pytest.mark.parametrize("name", REGIMES)
def test_fp64_round_trip_on_every_regime(name):
    assert _walk_round_trip(S.regime_case(name)) <= 1e-10


@pytest.mark.parametrize("ft,d", [(S.C2, 1), (("affine", "planar", "radial"), 3), (("radial", "planar"), 17),
                                  (("planar",) * 10, 32)])
def test_fp64_round_trip_on_random_chains(ft, d):
    assert _walk_round_trip(S.random_case(ft, d, 257, 11 + d, t_scale=1.0)) <= 1e-10


@pytest.mark.parametrize("ftype", ["planar", "radial", "affine"])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_jacobian_matches_autodiff(ftype, d):
    rng = np.random.default_rng(2000 + d)
    tk = rng.standard_normal((48, O.param_size(ftype, d)))
    z = rng.standard_normal((48, d)) * 1.5
    J = O.flow_jacobian(ftype, z, tk, d)
    assert J.shape == (48, d, d)
    ref = np.stack([torch.func.jacrev(lambda v: T_FWD[ftype](v, torch.as_tensor(ti, dtype=F64), d))(
        torch.as_tensor(zi, dtype=F64)).numpy() for zi, ti in zip(z, tk)])
    np.testing.assert_allclose(J, ref, rtol=1e-12, atol=1e-12)
    # its log|det| is the oracle's forward_log_det_jacobian
    _, fldj = O.flow_forward_fldj(ftype, z, tk, d)
    np.testing.assert_allclose(np.linalg.slogdet(J)[1], fldj, rtol=1e-10, atol=1e-10)
    # one parameter row against the batch, and one z against the batch
    np.testing.assert_array_equal(O.flow_jacobian(ftype, z, tk[:1], d)[0], O.flow_jacobian(ftype, z[:1], tk[:1], d)[0])
    np.testing.assert_array_equal(O.flow_jacobian(ftype, z[:1], tk, d)[5], O.flow_jacobian(ftype, z[:1], tk[5:6], d)[0])


def test_known_answers():
    d = 3
    rng = np.random.default_rng(6)
    B = 16
    eps = rng.standard_normal((B, d))
    # an affine-only chain over a trainable base: y = (loc + scale eps - shift) / (1 + t)
    t = rng.standard_normal((B, 4 * d))
    y, lp = O.chain_sample(eps, t, ("affine",), d, True)
    scale = 1e-3 + np.log1p(np.exp(math.log(math.e - 1) + 0.1 * t[:, d:2 * d]))
    x = t[:, :d] + scale * eps
    np.testing.assert_allclose(y, (x - t[:, 2 * d:3 * d]) / (1 + t[:, 3 * d:]), rtol=1e-13)
    want = (-0.5 * (eps ** 2).sum(1) - 0.5 * d * math.log(2 * math.pi) - np.log(scale).sum(1)
            + np.log(np.abs(1 + t[:, 3 * d:])).sum(1))
    np.testing.assert_allclose(lp, want, rtol=1e-12)
    # radial with t[1] = 0: beta = 0, the identity
    tk = rng.standard_normal((B, d + 2))
    tk[:, 1] = 0.0
    np.testing.assert_allclose(O.flow_inverse("radial", eps, tk, d), eps, atol=1e-15)
    # no flows over a fixed base returns eps; its log-density is N(0, I)'s
    y, lp = O.chain_sample(eps, np.zeros((B, 0)), (), d, False)
    np.testing.assert_array_equal(y, eps)
    np.testing.assert_allclose(lp, -0.5 * (eps ** 2).sum(1) - 0.5 * d * math.log(2 * math.pi), rtol=1e-14)
    # no flows over a trainable base: y = loc + scale eps
    t = rng.standard_normal((B, 2 * d))
    y, _ = O.chain_sample(eps, t, (), d, True)
    scale = 1e-3 + np.log1p(np.exp(math.log(math.e - 1) + 0.1 * t[:, d:]))
    np.testing.assert_allclose(y, t[:, :d] + scale * eps, rtol=1e-14)
    # planar, d = 1, u = 0, w = 1, b = 0: z_out = 0 has the root c = 0
    assert O.flow_inverse("planar", np.zeros((1, 1)), np.zeros((1, 3)), 1)[0, 0] == 0.0


def test_chain_sample_inverts_the_chain_and_broadcasts():
    ft, d = ("planar", "radial", "affine"), 3
    c = S.random_case(ft, d, 64, 9, t_scale=1.0)
    ym, ys = np.array([0.3, -1.0, 2.0], np.float32), np.array([0.5, 1.25, 2.0], np.float32)
    for mean, std in ((None, None), (ym, ys)):
        c["y_mean"], c["y_std"] = mean, std
        y, lp = O.chain_sample(c["eps"], c["t"], ft, d, True, mean, std)
        _, _, err, unit = S.backward_error(c, y)
        assert (err <= 1e-12).all() and (unit >= 2.0 ** -24).all()
        np.testing.assert_array_equal(lp, O.log_pdf(y, c["t"], ft, d, True, mean, std))
        y32, lp32 = O.chain_sample(c["eps"], c["t"], ft, d, True, mean, std, dtype=np.float32)
        assert y32.dtype == np.float32 and lp32.dtype == np.float32
        np.testing.assert_allclose(y32, y, rtol=1e-3, atol=1e-3)
    c["y_mean"] = c["y_std"] = None
    y, lp = O.chain_sample(c["eps"], c["t"], ft, d, True)
    y1, lp1 = O.chain_sample(c["eps"][:1], c["t"], ft, d, True)  # one eps row against B rows of t
    assert y1.shape == (64, d) and lp1.shape == (64,)
    np.testing.assert_array_equal(y1[0], y[0])
    yt, lpt = O.chain_sample(c["eps"], c["t"][:1], ft, d, True)  # one t row against B rows of eps
    np.testing.assert_array_equal(yt[0], y[0])
    np.testing.assert_array_equal(lpt[0], lp[0])
    # NaN inputs end the bisection and stay NaN
    e = c["eps"].copy()
    e[3, 1] = np.nan
    yn, lpn = O.chain_sample(e, c["t"], ft, d, True)
    assert np.isnan(yn[3]).any() and np.isnan(lpn[3]) and np.array_equal(np.delete(yn, 3, 0), np.delete(y, 3, 0))


@pytest.mark.parametrize("name", ["planar-steep-d1", "planar-steep_wide-d3", "planar-saturated-d1", "c2-steep-at4",
                                  "c2-saturated-at0"])
def test_backward_error_bound_rejects_a_root_stopped_short(name, monkeypatch):
    """The bound of the GPU test has teeth: the fp32 sampler whose planar bisection stops after 18
    halvings (a bracket of 2 |q| 2^-18, some 30 fp32 ulps of c) lands beyond 4 max(1, R_ref) units
    wherever the scalar map is not flat at the root."""
    case = S.regime_case(name)
    r_ref = S.reference_ratio(name, case)

    def short(z_out, u_hat, w, b):
        dt = z_out.dtype
        q = np.sum(w * u_hat, axis=-1, keepdims=True, dtype=dt)
        wzo = np.sum(w * z_out, axis=-1, keepdims=True, dtype=dt)
        lo, hi = wzo - np.abs(q), wzo + np.abs(q)
        for _ in range(18):
            mid = lo + dt.type(0.5) * (hi - lo)
            below = mid + q * np.tanh(mid + b) - wzo < 0
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        return z_out - u_hat * np.tanh(lo + dt.type(0.5) * (hi - lo) + b)

    monkeypatch.setattr(O, "planar_inverse", short)
    y, _ = O.chain_sample(case["eps"], case["t"], case["ft"], case["d"], True, dtype=np.float32)
    _, _, err, unit = S.backward_error(case, y)
    assert (err / unit).max() > 2 * 4.0 * max(1.0, r_ref)


# ---- the regimes are what they claim ------------------------------------------------------


@pytest.mark.parametrize("name", [n for n in REGIMES if n.startswith(("planar-", "c2-"))])
def test_planar_regime_conditions(name):
    case = S.regime_case(name)
    regime = name.split("-")[1]
    (lo, hi), _ = S.PLANAR_REGIMES[regime]
    q, arg = S.planar_stats(case)
    ft, d, k = case["ft"], case["d"], case["stressed"]
    blk = O.split_params(case["t"].astype(np.float64), ft, d, True)[1][k]
    wtu = ((1 + blk[:, d:2 * d]) * blk[:, :d]).sum(1)
    assert (wtu > lo - 1e-3).all() and (wtu < hi + 1e-3).all()
    assert case["t"].shape[0] == case["eps"].shape[0] == S.B_REGIME
    if regime.startswith("flat"):
        assert (q < -1 + 1.1e-5 + 1e-3).all() and (q >= -1).all()
        assert np.median(1 + q) < 2e-5  # w.u < -8: softplus(w.u) < 3.4e-4, and e^-14 for half of them
    if regime == "flat":
        assert (np.abs(arg) < 0.1).mean() >= 0.5
        # the slope of c + q tanh(c + b) at the root is tiny there
        assert np.median(1 + q * (1 - np.tanh(arg) ** 2)) < 1e-2
    if regime == "flat_wide":
        assert (np.abs(arg) > 1.0).mean() >= 0.5
    if regime.startswith("steep"):
        assert (q >= 1.1).all()
    if regime == "saturated":
        assert (np.abs(arg) > 9).mean() >= 0.5  # tanhf(9) == 1.0f


@pytest.mark.parametrize("name", [n for n in REGIMES if n.startswith("radial")])
def test_radial_regime_conditions(name):
    case = S.regime_case(name)
    ft, d = case["ft"], case["d"]
    K = len(ft)
    last = O.split_params(case["t"].astype(np.float64), ft, d, False)[1][K - 1]
    al, be, ga = O.radial_params(last, d)
    if "t0=-40" in name:
        assert (al < 1e-6).all() and (al > 5e-7).all()
    if "t0=40" in name:
        assert (np.abs(al - 10.0) < 1e-3).all()
    if "t1=-60" in name:
        assert (np.abs(be + 0.996) < 1e-3).all()
    A = S.radial_branch(case)
    sw = case["switch"]
    assert (A[sw] > 0).sum() >= sw.sum() // 8 and (A[sw] <= 0).sum() >= sw.sum() // 8  # both root branches
    assert (np.abs(A[sw]) <= 2e-3 * (al * (1 + be))[sw, 0] + 2.0 ** -23 * np.abs(ga[sw]).sum(1)).all()
    on = case["on_gamma"]
    assert on.sum() > 1000
    r0 = np.abs(case["eps"][on].astype(np.float64) - ga[on]).sum(1)
    assert (r0 == 0).all()
    if K == 1:
        y, _ = O.chain_sample(case["eps"], case["t"], ft, d, False)
        np.testing.assert_array_equal(y[on], ga[on])


@pytest.mark.parametrize("d", [1, 3])
def test_affine_regime_conditions(d):
    case = S.regime_case(f"affine-scales-d{d}")
    sc = 1.0 + O.split_params(case["t"].astype(np.float64), case["ft"], d, True)[1][0][:, d:]
    near = np.abs(sc - 1e-3) < 1e-7
    assert (near | (sc == -2.0)).all() and near.any() and (sc == -2.0).any()


def test_shape_matrix_covers_the_tiles():
    for name, (ft, d, B, rows, kw) in S.SHAPES.items():
        P = O.total_param_size(ft, d, kw.get("trainable", True))
        assert S.tile_rows(P) == rows, name
        assert B <= 4099 and (B % rows != 0 or name.startswith("a-")), name
        if name in S.EXPECT_P:
            assert P == S.EXPECT_P[name], name
    assert {S.tile_rows(O.total_param_size(ft, d, kw.get("trainable", True))) for ft, d, _, _, kw in S.SHAPES.values()} \
        == {256, 192, 128, 64, 32, 8}


# ---- the committed fixture ------------------------------------------------------------------


def test_golden_sample_fixture_rederives():
    g = load_golden("sample_stress_d1")
    assert g["flow_types"] == S.FIXTURE_FT and g["d"] == 1 and g["t"].shape == (257, 14) and g["eps"].shape == (257, 1)
    t, eps = S.stress_fixture_inputs()
    np.testing.assert_array_equal(t, g["t"])
    np.testing.assert_array_equal(eps, g["eps"])
    y64, lp64 = O.chain_sample(g["eps"], g["t"], g["flow_types"], 1, True)
    np.testing.assert_array_equal(y64, g["y64"])
    np.testing.assert_array_equal(lp64, g["lp64"])
    # the stored samples invert the chain: forward in fp64 lands on loc + scale eps
    case = dict(ft=g["flow_types"], d=1, trainable=True, eps=g["eps"], t=g["t"], y_mean=None, y_std=None)
    _, _, err, _ = S.backward_error(case, g["y64"])
    assert (err <= 1e-10).all()
    # the fp32 mirror's samples miss it by some finite number of backward-error units
    assert 0.0 < S.reference_ratio("fixture", case) < np.inf
