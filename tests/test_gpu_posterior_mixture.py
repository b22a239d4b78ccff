"""The Bayesian mixture estimators on the GPU: the fused posterior scores
(nfn_posterior_lse_gaussian_mixture_f32 / nfn_posterior_lse_kernel_mixture_f32) against the
fp64 numpy oracle (tests/posterior_mixture_oracle.py), and BayesMixtureDensityNetwork /
BayesKernelMixtureNetwork.

Shapes sit on the kernels' edges: ``(K, d)`` on the tile and waves-per-workgroup edges of
nfn_gmm.hip (tests/test_gpu_mdn.py), ``(M, d)`` on the (group width, values per lane)
instances of nfn_mixture.hip.  Batches straddle one wave tile (63 / 64 / 65) and take more
than one workgroup (257); S = 7 everywhere, S in {1, 2, 50} at B = 65 and 257.

Tolerance: the project's forward bound ``1e-5 * max(1, |ref64|)`` per element plus exact
agreement of the finite mask, for every input including the stress scalings (the fp32 mirror
of the whole posterior stays at or under 0.34 of that bound on these inputs)."""

import numpy as np
import pytest
import torch

from normalizingflownetwork_amd import (BayesKernelMixtureNetwork, BayesMixtureDensityNetwork, estimators, ops)
from normalizingflownetwork_amd.scorers import DummySklearWrapper, bayesian_log_likelihood_score

import posterior_mixture_oracle as PO
from mixture_cases import BASE, Gmm, Kernel, _dev, check, forward_variants, out_sum, refs, stress

pytestmark = pytest.mark.gpu

GMM_SHAPES = [(1, 1), (5, 1), (5, 3), (21, 1), (22, 1), (33, 1), (85, 1), (86, 1), (171, 1), (93, 5), (3, 32), (4, 1)]
KERNEL_SHAPES = [(1, 1), (6, 3), (63, 1), (64, 2), (65, 3), (100, 1), (129, 2), (300, 1), (1024, 8)]
# the (G, NV) instances of nfn_mixture.hip that KERNEL_SHAPES does not reach: G = 2, G = 4, (16, 1), (16, 2)
KERNEL_INSTANCES = [(2, 1), (3, 2), (12, 1), (24, 3)]
# S = 7 for every batch; S in {1, 2, 50} at B = 65 and 257
SIZES = [(B, 7) for B in (1, 63, 64, 65, 257)] + [(B, S) for B in (65, 257) for S in (1, 2, 50)]
GMM_STRESS = {"raw150": dict(raw_scale=150.0), "logits20": dict(logit_scale=20.0), "y30": dict(y_scale=30.0),
              "loc30": dict(loc_scale=30.0)}
KERNEL_STRESS = {"logits20": dict(logit_scale=20.0), "y30": dict(y_scale=30.0)}


@pytest.mark.parametrize("K,d", GMM_SHAPES)
@pytest.mark.parametrize("B,S", SIZES)
def test_gmm_parity(gpu, B, S, K, d):
    case = Gmm(B, K, d, S)
    forward_variants(case.tag, case)


@pytest.mark.parametrize("M,d", KERNEL_SHAPES)
@pytest.mark.parametrize("B,S", SIZES)
def test_kernel_parity(gpu, B, S, M, d):
    case = Kernel(B, M, d, S)
    forward_variants(case.tag, case)


def _single_draw_bitwise(case):
    """One draw without y_mean / y_std: the per-draw term IS the forward's computation."""
    dy, dr = _dev(case.y), _dev(case.rows)
    for mode in ("fast", "precise"):
        prev = ops.set_math_mode(mode)
        try:
            post = case.op(dy, dr[:1])[0].cpu().numpy()
            single = case.op(dy, dr[0])[0].cpu().numpy()
        finally:
            ops.set_math_mode(prev)
        assert post.tobytes() == single.tobytes(), f"{case.tag} {mode}"


@pytest.mark.parametrize("K,d", GMM_SHAPES)
@pytest.mark.parametrize("B", [65, 257])
def test_gmm_single_draw_is_bitwise_the_forward(gpu, B, K, d):
    _single_draw_bitwise(Gmm(B, K, d, 1))


@pytest.mark.parametrize("M,d", KERNEL_SHAPES)
@pytest.mark.parametrize("B", [65, 257])
def test_kernel_single_draw_is_bitwise_the_forward(gpu, B, M, d):
    _single_draw_bitwise(Kernel(B, M, d, 1))


@pytest.mark.parametrize("M,d", KERNEL_INSTANCES)
def test_kernel_every_instance(gpu, M, d):
    """The parity walk and the single-draw bitwise check (on the first of the two draws) on the
    smallest shapes that take the remaining instances and still straddle a wave tile."""
    case = Kernel(65, M, d, 2)
    assert np.isfinite(refs(case, case.y)[0]).all()
    forward_variants(case.tag, case)
    _single_draw_bitwise(case)


@pytest.mark.parametrize("K,d", GMM_SHAPES)
@pytest.mark.parametrize("kind", list(GMM_STRESS) + ["alternate-minus-inf"])
def test_gmm_stress(gpu, kind, K, d):
    case = Gmm(257, K, d, 7, **GMM_STRESS.get(kind, {}))
    ref = stress(f"{case.tag} stress {kind}", case, kind)
    if kind == "alternate-minus-inf" and K == 1:
        assert not np.isfinite(ref).any()  # the only component is removed in every draw
    else:
        assert np.isfinite(ref).all()


@pytest.mark.parametrize("M,d", KERNEL_SHAPES)
@pytest.mark.parametrize("kind", list(KERNEL_STRESS) + ["alternate-minus-inf"])
def test_kernel_stress(gpu, kind, M, d):
    case = Kernel(257, M, d, 7, **KERNEL_STRESS.get(kind, {}))
    ref = stress(f"{case.tag} stress {kind}", case, kind)
    if kind == "alternate-minus-inf" and M == 1:
        assert not np.isfinite(ref).any()
    else:
        assert np.isfinite(ref).all()


def _nonfinite_inputs(case):
    """Row 0: every draw all -inf logits.  Row 3: one draw all -inf.  Row 7: a +inf logit in one
    draw.  Row 64: a NaN in one draw."""
    rows, lg = case.rows, case.logits(case.rows)
    assert rows.shape[:2] == (4, 65)
    lg[:, 0, :] = -np.inf
    lg[2, 3, :] = -np.inf
    lg[1, 7, lg.shape[-1] // 2] = np.inf
    lg[3, 64, lg.shape[-1] - 1] = np.nan
    out, osum, nf = case.op(_dev(case.y), _dev(rows), want_nonfinite=True)
    got = out.cpu().numpy()
    bad = [int(i) for i in np.flatnonzero(~np.isfinite(got))]
    print(f"{case.tag}: non-finite rows {bad}, values {[float(got[i]) for i in (0, 3, 7, 64)]}, "
          f"out_sum = {osum.item()!r}, {nf.item()!r}")
    return got, bad, float(osum.item()), float(nf.item())


def _nonfinite(case):
    """A draw whose logits are all -inf has no component left: the posterior entries take its
    term as -inf, which drops out of the sum (the single-draw entries and the per-draw oracle
    give NaN there, -inf - -inf).  So row 0 is -inf, row 3 is finite (the other three draws, still
    - log 4), and the non-finite rows are exactly {0, 7, 64}.  Every other row is checked against
    the oracle as usual."""
    got, bad, osum, nf = _nonfinite_inputs(case)
    assert bad == [0, 7, 64]
    assert nf == 3.0
    assert not np.isfinite(osum)
    assert got[0] == -np.inf and np.isnan(got[64])
    others = case.ref(case.y[3:4], case.rows[[0, 1, 3], 3:4]) + np.log(3.0) - np.log(4.0)  # three draws, - log 4
    assert np.isfinite(others[0])
    assert abs(float(got[3]) - float(others[0])) <= BASE * max(1.0, abs(float(others[0])))
    rest = np.setdiff1d(np.arange(65), [0, 3])
    r64, r32 = refs(case, case.y)
    assert [int(i) for i in rest[~np.isfinite(r64[rest])]] == [7, 64]
    check(f"{case.tag} non-finite", got[rest], r64[rest], r32[rest])


@pytest.mark.parametrize("K,d", [(6, 3), (85, 1)])
def test_gmm_nonfinite_draws(gpu, K, d):
    _nonfinite(Gmm(65, K, d, 4))


@pytest.mark.parametrize("M,d", [(6, 3), (100, 1), (129, 2)])
def test_kernel_nonfinite_draws(gpu, M, d):
    _nonfinite(Kernel(65, M, d, 4))


@pytest.mark.parametrize("B,S", [(65, 7), (4099, 3)])
@pytest.mark.parametrize("K,d", [(5, 1), (93, 5)])
def test_gmm_out_sum(gpu, B, S, K, d):
    out_sum(Gmm(B, K, d, S))


@pytest.mark.parametrize("B,S", [(65, 7), (4099, 3)])
@pytest.mark.parametrize("M,d", [(6, 3), (100, 1), (1024, 8)])
def test_kernel_out_sum(gpu, B, S, M, d):
    out_sum(Kernel(B, M, d, S))


def test_layers_dispatch_to_their_ops(gpu):
    from normalizingflownetwork_amd import GaussianKernelsLayer, GaussianMixtureLayer, InverseNormalizingFlowLayer

    case = Gmm(65, 5, 2, 3)
    got = GaussianMixtureLayer(5, 2).posterior_lse(_dev(case.y), _dev(case.rows))[0]
    assert torch.equal(got, case.op(_dev(case.y), _dev(case.rows))[0])
    kc = Kernel(65, 6, 2, 3)
    layer = GaussianKernelsLayer(3, 2)
    layer.locs = kc.locs
    got, s, nf = layer.posterior_lse(_dev(kc.y), _dev(kc.rows), want_sum=True, want_nonfinite=True)
    want = ops.posterior_lse_kernel_mixture(_dev(kc.y), _dev(kc.rows), kc.locs, layer.scales("cuda"))[0]
    assert torch.equal(got, want) and nf.item() == 0.0
    assert s.item() == pytest.approx(float(want.double().sum().item()), rel=1e-12)
    flow = InverseNormalizingFlowLayer(("planar", "radial"), 1, trainable_base_dist=True)
    t = 0.3 * torch.randn((3, 65, flow.get_total_param_size()), generator=torch.Generator().manual_seed(1))
    y = torch.randn((65, 1), generator=torch.Generator().manual_seed(2))
    got = flow.posterior_lse(y, t)[0]
    assert torch.equal(got, ops.posterior_lse(y, t, flow.flow_types, 1, True)[0])


# --- estimators -------------------------------------------------------------------------

MODELS = {
    "mdn": lambda **kw: BayesMixtureDensityNetwork(n_dims=1, kl_weight_scale=0.01, n_centers=10, **kw),
    "kmn": lambda **kw: BayesKernelMixtureNetwork(n_dims=1, kl_weight_scale=0.01, n_centers=30, **kw),
}


def _line(n, d=1):
    x = np.linspace([-1.0] * d, [1.0] * d, n, dtype=np.float32).reshape((n, d))
    return x, x.copy()


def _prepared(kind, n=100, **kw):
    """An untrained model with its data normalisation (and the kernel centres) set: two calls
    with the same arguments give identical models."""
    x, y = _line(n)
    y = (y + 0.3 * np.sin(7.0 * x)).astype(np.float32)
    model = MODELS[kind](n_dims_x=1, **kw)
    model.set_data_normalization(x, y)
    if kind == "kmn":
        model.dist_layer.set_center_points((y - model.y_mean) / model.y_std, seed=22)
    return model, x, y


@pytest.mark.parametrize("kind", list(MODELS))
def test_big_bayesian_models(gpu, kind):
    """tests/test_bayesian_estimator.py:138-176 for the two mixture models."""
    x, y = _line(100)
    model = MODELS[kind](hidden_sizes=(32, 32), activation="tanh", learning_rate=3e-3, map_mode=False)
    model.fit(x, y, epochs=10, verbose=0)
    assert not np.isnan(model.evaluate(x, y))
    assert np.isfinite(model.score(x, y))


@pytest.mark.parametrize("kind", list(MODELS))
@pytest.mark.parametrize("d", [1, 3])
def test_model_output_dims(gpu, kind, d):
    """tests/test_bayesian_estimator.py:23-43 (test_model_output_dims_1d) for the mixture models."""
    x, y = _line(10, d)
    cls = BayesMixtureDensityNetwork if kind == "mdn" else BayesKernelMixtureNetwork
    m = cls(d, kl_weight_scale=1.0 / x.shape[0], n_centers=4, hidden_sizes=(16, 16))
    m.fit(x, y, epochs=1, verbose=0)
    output = m(x)
    assert output.event_shape == [d]
    assert output.batch_shape == [10]
    assert list(output.log_prob([[0.0] * d]).shape) == [10]
    assert list(m.pdf(x, y).shape) == [10]


@pytest.mark.parametrize("kind", list(MODELS))
def test_map_mode(gpu, kind):
    """tests/test_bayesian_estimator.py:109-135: the MAP model evaluates deterministically,
    the Bayesian model re-samples its weights per call (100 points: the kernel model's 30
    centres need that many)."""
    x, y = _line(100)
    m = MODELS[kind](hidden_sizes=(16, 16), noise_reg=("rule_of_thumb", 1.0), map_mode=True)
    m.fit(x, y, epochs=10, verbose=0)
    assert m.evaluate(x, y) == m.evaluate(x, y)
    b = MODELS[kind](hidden_sizes=(16, 16), noise_reg=("rule_of_thumb", 1.0), map_mode=False)
    b.fit(x, y, epochs=10, verbose=0)
    assert b.evaluate(x, y) != b.evaluate(x, y)


@pytest.mark.parametrize("kind", list(MODELS))
def test_map_mode_score_is_the_single_draw_mean(gpu, kind):
    m, x, y = _prepared(kind, map_mode=True)
    want = m(x).log_prob(y, m.y_mean, m.y_std).double().mean().item()
    assert m.score(x, y) == pytest.approx(want, rel=1e-5)
    assert m.last_score_nonfinite == 0


def _oracle_score(kind, model, y, t):
    layer = model.dist_layer
    if kind == "mdn":
        return PO.gmm_posterior(y, t, layer.n_centers, 1, model.y_mean, model.y_std).mean()
    return PO.kernel_posterior(y, t, layer.locs, layer.scales().cpu().numpy(), model.y_mean, model.y_std).mean()


@pytest.mark.parametrize("kind", list(MODELS))
def test_score_against_params_draws_through_the_oracle(gpu, kind):
    """score draws S networks; a fresh identically seeded model's params_draws gives the same
    S parameter tensors, pushed through the numpy oracle."""
    m, x, y = _prepared(kind, random_seed=5)
    got = m.score(x, y, n_draws=5)
    twin, _, _ = _prepared(kind, random_seed=5)
    t = twin.params_draws(x, 5).cpu().numpy()
    assert t.shape == (5, 100, m.dist_layer.get_total_param_size())
    assert np.abs(t[0] - t[1]).max() > 0.0  # the draws differ
    want = float(_oracle_score(kind, twin, y, t))
    print(f"{kind}: score {got:.9f}, oracle {want:.9f}")
    assert got == pytest.approx(want, rel=1e-5)


@pytest.mark.parametrize("kind", list(MODELS))
def test_chunked_score_shares_the_draws(gpu, kind, monkeypatch):
    """B = 300 in three chunks of 100 rows equals the unchunked score of an identically seeded
    model: the S networks are drawn once, only the order of the fp64 partial sums differs."""
    S = 5
    m, x, y = _prepared(kind, n=300)
    whole = m.score(x, y, n_draws=S)
    twin, _, _ = _prepared(kind, n=300)
    calls = []
    inner = twin.dist_layer.posterior_lse
    monkeypatch.setattr(twin.dist_layer, "posterior_lse",
                        lambda y_, t_, *a, **kw: (calls.append(tuple(t_.shape)), inner(y_, t_, *a, **kw))[1])
    P = twin.dist_layer.get_total_param_size()
    monkeypatch.setattr(estimators, "POSTERIOR_CHUNK_BYTES", 4 * S * P * 100)
    chunked = twin.score(x, y, n_draws=S)
    assert calls == [(S, 100, P)] * 3
    print(f"{kind}: whole {whole!r}, chunked {chunked!r}, rel diff {abs(whole - chunked) / abs(whole):.3e}")
    assert chunked == pytest.approx(whole, rel=1e-12)


@pytest.mark.parametrize("kind", list(MODELS))
def test_bayesian_scorer_is_the_model_score(gpu, kind):
    m, x, y = _prepared(kind)
    twin, _, _ = _prepared(kind)
    assert bayesian_log_likelihood_score(DummySklearWrapper(m), x, y) == twin.score(x, y)
