"""The pre-bound launchers (``ops.*Launcher``) and the density classes' ``log_prob_sum`` /
``log_prob_grid`` / result shapes.

A launcher marshals its arguments once and calls the same C entry as a functional op, so each
is compared BITWISE with that op on the same device tensors.  B = 130 is two full 64-row tiles
and a 2-row tail (ragged for the 32- and 16-row tiles too); layout A (P = 8, trainable base)
takes the 16-byte row path, layout B (P = 18, fixed base) the dword path with base offset 0."""

import numpy as np
import pytest
import torch

from normalizingflownetwork_amd import GaussianKernelsLayer, GaussianMixtureLayer, InverseNormalizingFlowLayer, ops
from oracle import nfn_oracle as O

pytestmark = pytest.mark.gpu

B = 130
LAYOUT_A = (("planar", "radial"), 1, True)
LAYOUT_B = (("planar", "radial", "affine"), 3, False)
LAYOUTS = [pytest.param(LAYOUT_A, id="A"), pytest.param(LAYOUT_B, id="B")]
H, S = 16, 3


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape and the same bits (a NaN equals the same NaN)."""
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits),
                                                                      b.contiguous().view(bits))


def _inputs(layout, gpu, draws=None):
    ft, d, tb = layout
    P = ops.total_param_size(ft, d, tb)
    gen = torch.Generator(device=gpu).manual_seed(7 * P + d)
    y = torch.randn((B, d), generator=gen, device=gpu)
    t = torch.randn((B, P) if draws is None else (draws, B, P), generator=gen, device=gpu)
    return y, t, P


def _dense_inputs(gpu, draws=None):
    ft, d, tb = LAYOUT_A
    P = ops.total_param_size(ft, d, tb)
    gen = torch.Generator(device=gpu).manual_seed(31)
    lead = () if draws is None else (draws,)
    y = torch.randn((B, d), generator=gen, device=gpu)
    h = torch.randn(lead + (B, H), generator=gen, device=gpu)
    W = torch.randn(lead + (H, P), generator=gen, device=gpu) / 4.0
    b = 0.1 * torch.randn(lead + (P,), generator=gen, device=gpu)
    return y, h, W, b, P


def _oracle_offsets(ft, d, tb):
    """Flow k's first column, read off the oracle's own split of a row of column numbers."""
    P = O.total_param_size(ft, d, tb)
    _, blocks = O.split_params(np.arange(P)[None, :], ft, d, tb)
    return [int(blk[0, 0]) for blk in blocks]


def _check_bind_sum(L, out, s, nf):
    target = torch.zeros((4,), dtype=torch.float64, device=out.device)
    L.bind_sum(target)
    L.launch()
    torch.cuda.synchronize()
    assert _same(L.out, out)
    assert _same(target[0:1], s) and _same(target[1:2], nf) and not target[2:4].any()
    assert L.sum.data_ptr() == target.data_ptr() and L.sum.shape == (1,)
    assert L.sum2.data_ptr() == target.data_ptr() and L.sum2.shape == (2,)
    assert L.nonfinite.data_ptr() == target[1:2].data_ptr()
    assert L.finish_sum().data_ptr() == target.data_ptr()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chain_launcher(gpu, layout):
    ft, d, tb = layout
    y, t, P = _inputs(layout, gpu)
    out, s, nf = ops.chain_log_prob(y, t, ft, d, tb, want_sum=True, want_nonfinite=True)
    L = ops.ChainLauncher(y, t, ft, d, tb)
    assert (L.B, L.P, L.fused_sum) == (B, P, True) and L.partials.numel() >= max(2, L.n_partials)
    L.launch()
    torch.cuda.synchronize()
    assert _same(L.out, out) and _same(L.sum2[0:1], s) and _same(L.sum2[1:2], nf)
    assert _same(L.finish_sum(), s) and _same(L.sum, s) and _same(L.nonfinite, nf)
    # partials only, finished by the reduction kernel: the same bits
    L2 = ops.ChainLauncher(y, t, ft, d, tb, fused_sum=False)
    L2.launch()
    got = L2.finish_sum()
    torch.cuda.synchronize()
    assert _same(L2.out, out) and _same(got, s) and _same(L2.sum2[0:1], s) and _same(L2.nonfinite, nf)
    with pytest.raises(AssertionError):
        L2.bind_sum(torch.zeros((2,), dtype=torch.float64, device=gpu))
    # the sum only
    L3 = ops.ChainLauncher(y, t, ft, d, tb, write_values=False)
    L3.launch()
    torch.cuda.synchronize()
    assert L3.out is None and _same(L3.sum, s) and _same(L3.nonfinite, nf)
    _check_bind_sum(L, out, s, nf)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chain_launcher_posterior(gpu, layout):
    ft, d, tb = layout
    y, t, P = _inputs(layout, gpu, draws=S)
    out, s, nf = ops.posterior_lse(y, t, ft, d, tb, want_sum=True, want_nonfinite=True)
    L = ops.ChainLauncher(y, t, ft, d, tb, draws=S)
    L.launch()
    torch.cuda.synchronize()
    assert (L.B, L.P) == (B, P)
    assert _same(L.out, out) and _same(L.sum2[0:1], s) and _same(L.sum2[1:2], nf)
    L2 = ops.ChainLauncher(y, t, ft, d, tb, draws=S, fused_sum=False)
    L2.launch()
    got = L2.finish_sum()
    torch.cuda.synchronize()
    assert _same(L2.out, out) and _same(got, s) and _same(L2.nonfinite, nf)
    _check_bind_sum(L, out, s, nf)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_grad_launcher(gpu, layout):
    ft, d, tb = layout
    y, t, P = _inputs(layout, gpu)
    g = torch.linspace(-1.0, 1.0, B, device=gpu)
    lp, gt, gy = ops.chain_log_prob_grad(y, t, ft, d, tb, g_out=g, want_logp=True)
    L = ops.GradLauncher(y, t, ft, d, tb, g_out=g, write_logp=True)
    L.launch()
    torch.cuda.synchronize()
    assert (L.B, L.P) == (B, P)
    assert _same(L.logp, lp) and _same(L.grad_t, gt) and _same(L.grad_y, gy)
    # no upstream gradient (ones), no log_prob
    _, gt1, gy1 = ops.chain_log_prob_grad(y, t, ft, d, tb)
    L1 = ops.GradLauncher(y, t, ft, d, tb)
    L1.launch()
    torch.cuda.synchronize()
    assert L1.logp is None and _same(L1.grad_t, gt1) and _same(L1.grad_y, gy1)


def test_dense_launcher(gpu):
    ft, d, tb = LAYOUT_A
    y, h, W, b, P = _dense_inputs(gpu)
    out, s, nf = ops.chain_log_prob_dense(y, h, W, b, ft, d, tb, want_sum=True, want_nonfinite=True)
    L = ops.DenseLauncher(y, h, W, b, ft, d, tb)
    L.launch()
    torch.cuda.synchronize()
    assert (L.B, L.P, L.H) == (B, P, H)
    assert _same(L.out, out) and _same(L.sum2[0:1], s) and _same(L.sum2[1:2], nf)
    assert _same(L.finish_sum(), s) and _same(L.sum, s) and _same(L.nonfinite, nf)
    L2 = ops.DenseLauncher(y, h, W, None, ft, d, tb, write_values=False)
    L2.launch()
    torch.cuda.synchronize()
    _, s2, nf2 = ops.chain_log_prob_dense(y, h, W, None, ft, d, tb, want_values=False, want_nonfinite=True)
    assert L2.out is None and _same(L2.sum, s2) and _same(L2.nonfinite, nf2)


def test_dense_grad_launcher(gpu):
    ft, d, tb = LAYOUT_A
    y, h, W, b, P = _dense_inputs(gpu)
    g = torch.linspace(-1.0, 1.0, B, device=gpu)
    _, gh, gW, gb, gy = ops.chain_log_prob_dense_grad(y, h, W, b, ft, d, tb, g_out=g)
    L = ops.DenseGradLauncher(y, h, W, b, ft, d, tb, g_out=g)
    L.launch()
    torch.cuda.synchronize()
    assert (L.B, L.P, L.H) == (B, P, H)
    assert _same(L.grad_h, gh) and _same(L.grad_W, gW) and _same(L.grad_b, gb) and _same(L.grad_y, gy)


def test_posterior_dense_launcher(gpu):
    ft, d, tb = LAYOUT_A
    y, h, W, b, P = _dense_inputs(gpu, draws=S)
    out, s, nf = ops.posterior_lse_dense(y, h, W, b, ft, d, tb, want_sum=True, want_nonfinite=True)
    L = ops.PosteriorDenseLauncher(y, h, W, b, ft, d, tb)
    L.launch()
    torch.cuda.synchronize()
    assert isinstance(L, ops.DenseLauncher) and (L.B, L.P, L.H, L.S) == (B, P, H, S)
    assert _same(L.out, out) and _same(L.sum2[0:1], s) and _same(L.sum2[1:2], nf)
    assert _same(L.finish_sum(), s) and _same(L.nonfinite, nf)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bijector_launcher(gpu, layout):
    ft, d, tb = layout
    z, t, P = _inputs(layout, gpu)
    z_ref, ldj_ref = ops.chain_forward_ldj(ft, z, t, _oracle_offsets(ft, d, tb), d)
    L = ops.BijectorLauncher(z, t, ft, d, tb)
    L.launch()
    torch.cuda.synchronize()
    assert L.B == B and _same(L.z_out, z_ref) and _same(L.ldj, ldj_ref)


@pytest.mark.parametrize("params", ["views", "separate", "strided"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_flows_launcher(gpu, layout, params):
    ft, d, tb = layout
    z, t, P = _inputs(layout, gpu)
    offs = _oracle_offsets(ft, d, tb)
    zk, ldjs = z, []
    for f, o in zip(ft, offs):
        zk, l = ops.flow_forward_ldj(f, zk, t[:, o:o + ops.param_size(f, d)].contiguous(), d)
        ldjs.append(l)
    L = ops.FlowsLauncher(z, t, ft, d, tb, params=params)
    assert L.mode == params and L.B == B and L.bytes_per_launch > 0  # at these shapes the split pays
    assert len(L.params) == (0 if params == "strided" else len(ft))
    L.launch()
    torch.cuda.synchronize()
    assert _same(L.z_out, zk)
    assert L.ldj.shape == (len(ft), B)
    for k, l in enumerate(ldjs):
        assert _same(L.ldj[k], l), f"ldj of flow {k}"
    assert ops.FlowsLauncher(z, t, ft, d, tb, separate=True).mode == "separate"


# ---------------------------------------------------------------------------
# The three density classes
# ---------------------------------------------------------------------------

def _flow_dist(t):
    ft, d, tb = LAYOUT_A
    return InverseNormalizingFlowLayer(ft, d, trainable_base_dist=tb)(t)


def _kernel_layer():
    layer = GaussianKernelsLayer(3, 2, init_scales=(0.3, 0.7))
    layer.set_center_points(np.random.default_rng(3).standard_normal((40, 2)))
    return layer


def _kernel_dist(t):
    return _kernel_layer()(t)


def _gmm_dist(t):
    return GaussianMixtureLayer(3, 2)(t)


# (make a distribution of t, row width W, event size d)
DENSITIES = [pytest.param((_flow_dist, 8, 1), id="flows"), pytest.param((_kernel_dist, 6, 2), id="kernel_mixture"),
             pytest.param((_gmm_dist, 15, 2), id="gaussian_mixture")]


def _density_inputs(gpu, W, d, n=B):
    gen = torch.Generator(device=gpu).manual_seed(11 * W + d)
    return torch.randn((n, d), generator=gen, device=gpu), torch.randn((n, W), generator=gen, device=gpu)


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("poison", [False, True], ids=["finite", "one-nan"])
def test_log_prob_sum(gpu, density, poison):
    make, W, d = density
    y, t = _density_inputs(gpu, W, d)
    if poison:
        t[5, 0] = float("nan")
    dist = make(t)
    lp = dist.log_prob(y)
    assert lp.shape == (B,)
    s, nf = dist.log_prob_sum(y, want_nonfinite=True)
    assert s.dtype == torch.float64 and s.shape == () and nf.shape == ()
    bad = int((~torch.isfinite(lp)).sum().item())
    assert bad == (1 if poison else 0)
    assert int(nf.item()) == bad
    assert _same(dist.log_prob_sum(y), s)
    ref = lp.double().sum()
    if poison:
        assert not torch.isfinite(s) and not torch.isfinite(ref)
    else:
        bound = B * 2.0 ** -52 * lp.double().abs().sum().item()  # fp64 summation of the same fp32 values
        err = abs(s.item() - ref.item())
        print(f"log_prob_sum: |err| = {err:.3e}, bound = {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("density", DENSITIES)
def test_log_prob_grid(gpu, density):
    make, W, d = density
    _, t = _density_inputs(gpu, W, d)
    dist = make(t)
    y_grid = torch.randn((3, d), generator=torch.Generator(device=gpu).manual_seed(5), device=gpu)
    grid = dist.log_prob_grid(y_grid)
    assert grid.shape == (3, B)
    for g in range(3):
        assert _same(grid[g], dist.log_prob(y_grid[g:g + 1])), f"grid row {g}"
    assert _same(dist.prob_grid(y_grid), torch.exp(grid))
    # a batch of rank 2: (G, *batch_shape)
    assert make(t[:120].reshape(4, 30, W)).log_prob_grid(y_grid).shape == (3, 4, 30)


@pytest.mark.parametrize("density", DENSITIES)
def test_log_prob_result_shapes(gpu, density):
    make, W, d = density
    y, t = _density_inputs(gpu, W, d, n=10)
    flat = make(t).log_prob(torch.cat([y[:5], y[:5]]))  # row (i, j) of the (2, 5) batch is t[5 i + j], y[j]
    dist = make(t.reshape(2, 5, W))
    assert dist.batch_shape == (2, 5) and dist.event_shape == (d,) and dist.params.shape == (2, 5, W)
    lp = dist.log_prob(y[:5])
    assert lp.shape == (2, 5) and _same(lp.reshape(-1), flat)
    assert _same(dist.prob(y[:5]), torch.exp(lp))
    one = make(t[0]).log_prob(y[0])
    assert one.shape == () and _same(one.reshape(1), flat[:1])
    rows = make(t[:1]).log_prob(y[:7])
    assert rows.shape == (7,) and _same(rows[:1], flat[:1])


@pytest.mark.parametrize("density", DENSITIES)
def test_log_prob_takes_the_differentiable_path(gpu, density):
    make, W, d = density
    y, t = _density_inputs(gpu, W, d, n=10)
    assert make(t).log_prob(y).grad_fn is None
    plain = make(t).log_prob(y)
    lp = make(t.clone().requires_grad_(True)).log_prob(y)
    assert lp.grad_fn is not None and _same(lp.detach(), plain)
    with torch.no_grad():
        assert make(t.clone().requires_grad_(True)).log_prob(y).grad_fn is None


def test_kernel_mixture_scales_alone_take_the_differentiable_path(gpu):
    y, t = _density_inputs(gpu, 6, 2, n=10)
    layer = _kernel_layer()
    (v,) = layer.trainable_parameters(gpu)
    assert v.requires_grad and not t.requires_grad
    lp = layer(t).log_prob(y)
    assert lp.grad_fn is not None
    lp.sum().backward()
    assert v.grad is not None and v.grad.shape == (2,)
