"""Kernel mixture network on the GPU: the fused mixture log_prob (nfn_kernel_mixture_logprob_f32)
and its backward against the fp64 numpy oracle (tests/mixture_oracle.py), the autograd op,
and the KernelMixtureNetwork estimator.

Tolerances.  Forward and the ordinary-input gradients: the project's base bound
``1e-5 * max(1, |ref64|)`` (``grad_scales``, a batch sum, against its conditioning
``1e-5 * max(1, sum_b |term_bk|)``).  Gradients on the two stress inputs (posterior weights are
exponentials of differences of numbers near 1e4, where the fp32 mirror itself is over the plain
bound): each array at ``1e-5 * max(1, |ref64|) + 4 * max|ref32 - ref64|``."""

import numpy as np
import pytest
import torch

from normalizingflownetwork_amd import GaussianKernelsLayer, KernelMixtureNetwork, ops

import mixture_oracle as MO
from mixture_cases import (BASE, Kernel, _dev, check_grads, check_op, forward_variants, gradient_walk, nonfinite_rows,
                           out_sum, stress)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (6, 3), (63, 1), (64, 2), (65, 3), (100, 1), (129, 2), (1024, 8)]
BATCHES = [1, 63, 64, 65, 257, 4099]
GRAD_BATCHES = [1, 65, 257]


@pytest.mark.parametrize("M,d", SHAPES)
@pytest.mark.parametrize("B", BATCHES)
def test_forward_parity(gpu, B, M, d):
    forward_variants(f"mixture B={B} M={M} d={d}", Kernel(B, M, d))


@pytest.mark.parametrize("M,d", [(3, 2), (12, 1), (24, 3), (200, 2), (300, 1), (600, 4)])
def test_every_kernel_instance(gpu, M, d):
    """Component counts that take the (group width, values per lane) instances the shapes above
    do not reach, forward and gradients."""
    B = 65
    case = Kernel(B, M, d, seed=2)
    check_op(f"mixture instance M={M} d={d}", case)
    g = np.random.default_rng(M).standard_normal(B).astype(np.float32)
    _check_grads(f"mixture instance grad M={M} d={d}", case, g)


STRESS = {"logits20": dict(logit_scale=20.0), "y30": dict(y_scale=30.0)}
STRESS_SHAPES = [(6, 3), (100, 1), (1024, 8)]


@pytest.mark.parametrize("M,d", STRESS_SHAPES)
@pytest.mark.parametrize("kind", ["logits20", "y30", "alternate-minus-inf"])
def test_forward_stress(gpu, kind, M, d):
    ref = stress(f"mixture stress {kind} M={M} d={d}", Kernel(257, M, d, seed=3, **STRESS.get(kind, {})), kind)
    assert np.isfinite(ref).all()
    if kind == "y30":
        assert np.abs(ref).max() > 1e3


@pytest.mark.parametrize("M,d", [(6, 3), (100, 1), (129, 2)])
def test_nonfinite_rows_and_count(gpu, M, d):
    case = Kernel(65, M, d, seed=4)
    case.rows[0, :] = -np.inf
    case.rows[7, M // 2] = np.inf
    case.rows[64, M - 1] = np.nan
    nonfinite_rows(f"mixture non-finite M={M} d={d}", case, [0, 7, 64])


@pytest.mark.parametrize("B,M,d", [(65, 6, 3), (4099, 100, 1), (4099, 1024, 8)])
def test_out_sum(gpu, B, M, d):
    out_sum(Kernel(B, M, d, seed=5))


# --- gradients --------------------------------------------------------------------------

def _check_grads(what, case, g, ym=None, ys=None, widened=False):
    """The shared check, and grad_scales (a batch sum finished in fixed order) bitwise equal
    between two runs."""
    gl, gy, gs = check_grads(what, case, g, ym, ys, widened)
    assert gs.tobytes() == case.grad(g, ym, ys)[3].tobytes(), "grad_scales differs between two runs"
    return gl, gy, gs


@pytest.mark.parametrize("M,d", SHAPES)
@pytest.mark.parametrize("B", GRAD_BATCHES)
def test_gradient_parity(gpu, B, M, d):
    g = np.random.default_rng(B + M).standard_normal(B).astype(np.float32)
    gradient_walk(f"mixture grad B={B} M={M} d={d}", Kernel(B, M, d, seed=6), g, check=_check_grads)


@pytest.mark.parametrize("M,d", STRESS_SHAPES)
@pytest.mark.parametrize("kind", ["logits20", "y30"])
def test_gradient_stress(gpu, kind, M, d):
    """Gated at 1e-5 max(1, |ref64|) + 4 max|ref32 - ref64| per array (module docstring)."""
    B = 257
    g = np.random.default_rng(M).standard_normal(B).astype(np.float32)
    _check_grads(f"mixture grad stress {kind} M={M} d={d}", Kernel(B, M, d, seed=7, **STRESS[kind]), g, widened=True)


def test_autograd_matches_grad_entry(gpu):
    B, M, d = 65, 100, 2
    case = Kernel(B, M, d, seed=8)
    y, t, locs, s = case.y, case.rows, case.locs, case.scales
    g = np.random.default_rng(1).standard_normal(B).astype(np.float32)
    dy, dt, ds = (_dev(a).requires_grad_(True) for a in (y, t, s))
    lp = ops.kernel_mixture_log_prob_diff(dy, dt, _dev(locs), ds)
    (lp * _dev(g)).sum().backward()
    _, gl, gy, gs = case.grad(g)
    np.testing.assert_array_equal(dt.grad.cpu().numpy(), gl)
    np.testing.assert_array_equal(dy.grad.cpu().numpy(), gy)
    np.testing.assert_array_equal(ds.grad.cpu().numpy(), gs)
    # y broadcast from one row: its gradient is the batch sum
    dy1 = _dev(y[:1]).requires_grad_(True)
    ops.kernel_mixture_log_prob_diff(dy1, _dev(t), _dev(locs), _dev(s)).sum().backward()
    ref = MO.log_prob_grads(y[:1], t, locs, s)[1].sum(0, keepdims=True)
    np.testing.assert_allclose(dy1.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)


def test_gradient_wrt_bandwidth_variable(gpu):
    """d/dv through the layer: the fused grad_scales mapped through the sigmoid and summed over
    each scale's block by torch, against fp64 autograd through the torch composition."""
    B, d, nc = 257, 2, 25
    layer = GaussianKernelsLayer(nc, d)
    M = layer.get_total_param_size()
    y, t, locs, _ = MO.make_inputs(B, M, d, seed=9)
    layer.locs = locs
    (v,) = layer.trainable_parameters(torch.device("cuda", 0))
    with torch.no_grad():
        v.copy_(torch.tensor([0.3, -0.2]))
    layer.train_log_prob(_dev(y), _dev(t)).sum().backward()
    got = v.grad.cpu().numpy().astype(np.float64)
    layer.finish_training()
    v64 = torch.tensor([0.3, -0.2], dtype=torch.float64, requires_grad=True)
    off = torch.tensor(np.log(np.expm1(np.float64(layer.init_scales))))
    s64 = (torch.nn.functional.softplus(v64) + off).repeat_interleave(nc)
    ty, tt, tl = (torch.from_numpy(np.asarray(a, np.float64)) for a in (y, t, locs))
    z2 = (((ty[:, None, :] - tl[None]) / s64[None, :, None]) ** 2).sum(-1)
    c = -0.5 * z2 - d * torch.log(s64.abs())[None, :] - 0.5 * d * np.log(2 * np.pi)
    (torch.logsumexp(tt + c, -1) - torch.logsumexp(tt, -1)).sum().backward()
    cond = MO.log_prob_grads(y, t, locs, s64.detach().numpy())[3]
    sig = 1.0 / (1.0 + np.exp(-np.array([0.3, -0.2])))
    bound = sig * (BASE * np.maximum(1.0, cond)).reshape(2, nc).sum(1)
    err = np.abs(got - v64.grad.numpy())
    print(f"dv: err / bound = {err / bound}")
    assert (err <= bound).all()


# --- estimator --------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3])
def test_model_output_dims(gpu, d):
    """tests/test_ml_estimator.py:19-40, 87-102 for the kernel mixture network."""
    x = np.linspace([-1.0] * d, [1.0] * d, 10).reshape((10, d))
    y = np.linspace([-1.0] * d, [1.0] * d, 10).reshape((10, d))
    model = KernelMixtureNetwork(d, n_centers=3, hidden_sizes=(2, 2))
    model.fit(x, y, epochs=1, verbose=0)
    output = model(x)
    assert output.event_shape == [d]
    assert output.batch_shape == [10]
    lp = output.log_prob([[0.0] * d])
    assert list(lp.shape) == [10] and torch.isfinite(lp).all()


def _bimodal(n, rng):
    x = np.linspace(-3, 3, n, dtype=np.float32).reshape((n, 1))
    y = (np.where(rng.random(n) < 0.5, 3.0, -3.0) + 0.5 * rng.standard_normal(n)).astype(np.float32).reshape((n, 1))
    return x, y


def test_short_fit_on_bimodal_data(gpu):
    x, y = _bimodal(400, np.random.default_rng(22))
    model = KernelMixtureNetwork(1, n_centers=25, hidden_sizes=(10, 10))
    hist = model.fit(x, y, epochs=40, verbose=0)["loss"]
    assert len(hist) == 40 and hist[-1] < hist[0]
    score = model.score(x, y)
    gauss = -0.5 * np.log(2 * np.pi * np.var(y.astype(np.float64))) - 0.5  # one Gaussian fitted to y
    print(f"KMN score {score:.4f}, single Gaussian {gauss:.4f}, loss {hist[0]:.4f} -> {hist[-1]:.4f}")
    assert score > gauss
    assert score == pytest.approx(-model.evaluate(x, y), rel=1e-5)


def test_fit_graph_replay_matches_eager(gpu):
    """The captured training step (MLP, fused mixture forward / backward, the bandwidth
    variable's update) replays exactly as the eager loop trains."""
    x, y = _bimodal(203, np.random.default_rng(5))  # 6 full batches of 32 + a partial one per epoch
    out = {}
    for use_graph in (True, False):
        m = KernelMixtureNetwork(1, n_centers=10, hidden_sizes=(16, 16), noise_reg=("fixed_rate", 0.1))
        hist = m.fit(x, y, epochs=4, verbose=0, use_graph=use_graph)["loss"]
        out[use_graph] = (hist, [w.detach().cpu().numpy() for w in m._mlp.weights + m._mlp.biases + [m.dist_layer.v]])
    assert out[True][0] == out[False][0]
    for a, b in zip(out[True][1], out[False][1]):
        np.testing.assert_array_equal(a, b)
    assert np.abs(out[True][1][-1]).max() > 0  # the bandwidth variable trained


def test_density_heatmap_on_a_kernel_mixture(gpu):
    from normalizingflownetwork_amd.flow_plotting import model_density_heatmap

    x, y = _bimodal(120, np.random.default_rng(3))
    model = KernelMixtureNetwork(1, n_centers=8, hidden_sizes=(8, 8))
    model.fit(x, y, epochs=2, verbose=0)
    xs = x[::10]
    heat = model_density_heatmap(xs, model, (-5.0, 5.0), y_num=20)
    assert heat.shape == (20, len(xs))
    grid = np.linspace(5.0, -5.0, num=20)
    for r in (0, 7, 19):
        pdf = model.pdf(xs, np.full((len(xs), 1), grid[r], np.float32)).cpu().numpy()
        np.testing.assert_allclose(heat[r], pdf, rtol=1e-4, atol=1e-9)
