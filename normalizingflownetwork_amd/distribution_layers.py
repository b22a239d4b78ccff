"""``InverseNormalizingFlowLayer`` and the flow distribution it produces.

Drop-in for ``estimators/DistributionLayers.py:215-294``.  The reference builds
``tfd.TransformedDistribution(MVNDiag(base(t)), Invert(Chain(reversed flows)))``
per call and TF evaluates its ``log_prob`` as ~40 eager element-wise ops per
flow.  Here the same object graph exists for API compatibility (``.bijector``,
``.distribution``, ``event_shape``, ``batch_shape``, the reversed-order
``_get_bijector``), but ``log_prob`` / ``prob`` go straight to ONE fused HIP
kernel (``nfn_chain_logprob_f32``) that walks the whole chain per sample in
registers.
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .normalizing_flows import FLOWS, Chain, Invert
from .normalizing_flows.flows import SplitBlocks, snapshot_rows


class TensorShape(tuple):
    """Shape tuple that compares equal to lists / tuples / torch.Size (as TF's
    ``TensorShape`` does in the reference tests, e.g. ``dist.event_shape == [1]``)."""

    def __eq__(self, other):
        if isinstance(other, (list, tuple)):
            return tuple(self) == tuple(other)
        if isinstance(other, (int, np.integer)):
            return len(self) == 1 and self[0] == int(other)
        return NotImplemented

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    __hash__ = tuple.__hash__


def _shape(x):
    s = getattr(x, "shape", None)
    return tuple(np.shape(x)) if s is None else tuple(s)


def _cols(t, begin: int, end: int):
    """``t[..., begin:end]`` for torch tensors (a view: no copy), numpy arrays and lists."""
    if isinstance(t, torch.Tensor):
        return t[..., begin:end]
    return np.asarray(t, dtype=np.float32)[..., begin:end]


def _needs_grad(*xs) -> bool:
    return torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad for x in xs)


def _broadcast_rows(y, t, event: int, width: int):
    """Bring ``y (..., event)`` and ``t (..., width)`` to 2-D row form for the kernel.

    The 2-D case (including batch-1 broadcast either way) passes through with
    stride-0 broadcasting inside the kernel; other batch ranks are expanded."""
    y = ops.as_device_f32(y)
    t = ops.as_device_f32(t) if width > 0 else None
    if y.dim() == 1:
        y = y.unsqueeze(0)
    bt = tuple(t.shape[:-1]) if t is not None else ()
    if t is not None and t.dim() == 1:
        t = t.unsqueeze(0)
    if y.dim() == 2 and (t is None or t.dim() == 2):
        return y, t, None
    bshape = torch.broadcast_shapes(tuple(y.shape[:-1]), bt)
    y2 = y.expand(*bshape, event).reshape(-1, event)
    t2 = t.expand(*bshape, width).reshape(-1, width) if t is not None else None
    return y2, t2, bshape


class MultivariateNormalDiag:
    """Base distribution of the layer (``DistributionLayers.py:280-294``).

    ``log_prob`` runs the fused kernel with an empty flow chain."""

    def __init__(self, t, n_dims: int, trainable: bool):
        self._t = t
        self._n_dims = int(n_dims)
        self._trainable = bool(trainable)
        if trainable:
            assert _shape(t)[-1] >= 2 * n_dims

    @property
    def event_shape(self):
        return TensorShape([self._n_dims])

    @property
    def batch_shape(self):
        return TensorShape(_shape(self._t)[:-1])

    def log_prob(self, x):
        d = self._n_dims
        base = _cols(self._t, 0, 2 * d) if self._trainable else None
        y, t, bshape = _broadcast_rows(x, base if base is not None else np.zeros((1, 0), np.float32), d,
                                       2 * d if self._trainable else 0)
        if not self._trainable:
            B = max(y.shape[0], int(np.prod(self.batch_shape)) if len(self.batch_shape) else 1)
            y = y.expand(B, d) if y.shape[0] == 1 and B > 1 else y
        if _needs_grad(y, t):
            lp = ops.log_prob(y, t, (), d, self._trainable)
        else:
            lp, _ = ops.chain_log_prob(y, t, (), d, self._trainable)
        return lp if bshape is None else lp.reshape(bshape)

    def prob(self, x):
        return torch.exp(self.log_prob(x))


class _RowDensity:
    """A conditional density whose parameters are the rows of ``t (..., width)``, evaluated by
    fused kernels over 2-D rows.  A subclass supplies ``_forward`` (its forward op, no
    autograd), ``_diff`` (its differentiable op) and, beyond ``t``, the tensors that may
    require grad (``_grad_inputs``)."""

    def __init__(self, t, n_dims: int):
        self._t = t
        self._n_dims = int(n_dims)

    def _forward(self, y, t, y_mean, y_std, **want):
        """The forward op on rows: ``(log_prob | None, sum | None[, non-finite count])``."""
        raise NotImplementedError

    def _diff(self, y, t, y_mean, y_std) -> torch.Tensor:
        """The differentiable op on rows: ``log_prob`` (B,) with the fused backward behind it."""
        raise NotImplementedError

    def _grad_inputs(self) -> tuple:
        return ()

    @property
    def _width(self) -> int:
        return _shape(self._t)[-1]

    @property
    def event_shape(self):
        return TensorShape([self._n_dims])

    @property
    def batch_shape(self):
        return TensorShape(_shape(self._t)[:-1])

    @property
    def params(self):
        return self._t

    def log_prob(self, y, y_mean=None, y_std=None):
        """``log_prob(y)``; optional fused normalisation ``(y-mean)/std`` with the
        ``-sum(log std)`` Jacobian correction (``BaseEstimator.py:85-86``)."""
        yy, tt, bshape = _broadcast_rows(y, self._t, self._n_dims, self._width)
        if _needs_grad(yy, tt, *self._grad_inputs()):  # training: the fused backward kernel
            lp = self._diff(yy, tt, y_mean, y_std)
        else:
            lp, _ = self._forward(yy, tt, y_mean, y_std)
        if bshape is not None:
            return lp.reshape(bshape)
        if len(self.batch_shape) == 0 and _shape(y) and len(_shape(y)) == 1:
            return lp.reshape(())
        return lp

    def prob(self, y, y_mean=None, y_std=None):
        return torch.exp(self.log_prob(y, y_mean, y_std))

    def log_prob_sum(self, y, y_mean=None, y_std=None, want_nonfinite: bool = False):
        """``sum_b log_prob(y_b)`` in fp64, reduced on the device (no (B,) output written);
        with ``want_nonfinite`` also the number of non-finite log-densities (fp64 scalar)."""
        yy, tt, _ = _broadcast_rows(y, self._t, self._n_dims, self._width)
        _, s, nf = self._forward(yy, tt, y_mean, y_std, want_values=False, want_nonfinite=True)
        return (s[0], nf[0]) if want_nonfinite else s[0]

    def _grid_rows(self, y_grid):
        """``(y_grid (G, d), t (B, width), batch shape)`` of a density grid."""
        t = ops.as_device_f32(self._t)
        t2 = t if t.dim() == 2 else t.reshape(-1, self._width)
        return ops.as_device_f32(y_grid).reshape(-1, self._n_dims), t2, tuple(t.shape[:-1])

    def log_prob_grid(self, y_grid, y_mean=None, y_std=None) -> torch.Tensor:
        """``log_prob`` of each grid value (G, d) under every batch member: (G, *batch_shape).
        One launch per grid row, its ``y`` broadcast over the batch (a plotting path)."""
        yg, t2, bshape = self._grid_rows(y_grid)
        with torch.no_grad():
            rows = [self._forward(yg[g:g + 1], t2, y_mean, y_std)[0] for g in range(yg.shape[0])]
        return torch.stack(rows).reshape((yg.shape[0],) + bshape)

    def prob_grid(self, y_grid, y_mean=None, y_std=None) -> torch.Tensor:
        return torch.exp(self.log_prob_grid(y_grid, y_mean, y_std))


class FlowDistribution(_RowDensity):
    """``TransformedDistribution(base, Invert(Chain(...)))`` of the reference,
    evaluated by the fused kernel."""

    def __init__(self, t, n_dims: int, flow_types: Sequence[str], trainable_base_dist: bool):
        super().__init__(t, n_dims)
        self._flow_types = tuple(flow_types)
        self._trainable = bool(trainable_base_dist)
        self.distribution = InverseNormalizingFlowLayer._get_base_dist(t, n_dims, trainable_base_dist)
        # A wrong width raises AssertionError at construction, as in the reference
        # (DistributionLayers.py:272); the Chain itself (and the parameter snapshot its flows
        # own) is built on first use of ``bijector``: log_prob never needs it.
        flow_w = _shape(t)[-1] - (2 * n_dims if trainable_base_dist else 0)
        assert sum(FLOWS[f].get_param_size(n_dims) for f in self._flow_types) == flow_w
        self._bijector = None

    @property
    def bijector(self):
        """``Invert(Chain(flows))`` over a snapshot of ``t``'s flow columns taken on FIRST
        ACCESS (``_get_bijector``), not at construction: ``log_prob`` never pays for the copy.
        The distribution itself reads ``t`` live — ``log_prob`` / ``prob`` evaluate ``t`` as it
        is at the call, and so does the snapshot when it is taken — so a write into ``t``
        between construction and that first access reaches both (TF's tensors are immutable,
        so the reference has no such window).  From then on the Chain keeps its snapshot."""
        if self._bijector is None:
            d = self._n_dims
            # built under grad mode whenever t requires grad: a Chain first touched under
            # torch.no_grad() (sampling) is cached, and later forward / fldj calls must still
            # differentiate into t
            with torch.set_grad_enabled(isinstance(self._t, torch.Tensor) and self._t.requires_grad):
                flow_t = _cols(self._t, 2 * d, _shape(self._t)[-1]) if self._trainable else self._t
                self._bijector = Invert(InverseNormalizingFlowLayer._get_bijector(flow_t, self._flow_types, d))
        return self._bijector

    def _forward(self, y, t, y_mean, y_std, **want):
        return ops.chain_log_prob(y, t, self._flow_types, self._n_dims, self._trainable, y_mean, y_std, **want)

    def _diff(self, y, t, y_mean, y_std):
        return ops.log_prob(y, t, self._flow_types, self._n_dims, self._trainable, y_mean, y_std)

    def log_prob_grid(self, y_grid, y_mean=None, y_std=None) -> torch.Tensor:
        """``log_prob`` of each grid value (G, d) under every batch member: (G, *batch_shape),
        by the grid kernel (one launch)."""
        yg, t2, bshape = self._grid_rows(y_grid)
        out = ops.chain_log_prob_grid(yg, t2, self._flow_types, self._n_dims, self._trainable, y_mean, y_std)
        return out.reshape((yg.shape[0],) + bshape)

    def sample(self, sample_shape=(), seed=None) -> torch.Tensor:
        """Draws of shape ``sample_shape + batch_shape + [d]`` through the inverted flows
        (``nfn_chain_sample_f32``).  An extension: the reference's layer cannot sample
        (``DistributionLayers.py:223-226, 240``) because its flows define no inverse."""
        return self.sample_and_log_prob(sample_shape, seed)[0]

    def sample_and_log_prob(self, sample_shape=(), seed=None):
        d = self._n_dims
        P = _shape(self._t)[-1]
        t = ops.as_device_f32(self._t) if P > 0 else None
        bshape = tuple(self.batch_shape)
        sshape = (sample_shape,) if isinstance(sample_shape, int) else tuple(sample_shape)
        n_s = int(np.prod(sshape)) if sshape else 1
        nb = int(np.prod(bshape)) if bshape else 1
        dev = ops._device()
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed) if seed is not None else int(torch.randint(0, 2**62, (1,)).item()))
        eps = torch.randn((n_s * nb, d), generator=gen, device=dev)
        if t is not None:
            t2 = t.reshape(nb, P)
            t2 = t2.repeat(n_s, 1) if n_s > 1 else t2
        else:
            t2 = torch.zeros((1, 0), dtype=torch.float32, device=dev)
        y, lp = ops.chain_sample(eps, t2, self._flow_types, d, self._trainable)
        return y.reshape(sshape + bshape + (d,)), lp.reshape(sshape + bshape)


class InverseNormalizingFlowLayer:
    """Turns a parameter tensor ``t`` into a flow distribution.

    ``flow_types`` are applied base -> transformed distribution; the layer
    evaluates ``log_prob`` of externally provided data by inverting the chain.
    Mirrors ``estimators/DistributionLayers.py:215-265`` (a Keras
    ``DistributionLambda`` there; a plain callable here)."""

    _flow_types = None
    _trainable_base_dist = None
    _n_dims = None

    def __init__(self, flow_types, n_dims, trainable_base_dist=False):
        assert all([flow_type in FLOWS for flow_type in flow_types])
        self._flow_types = tuple(flow_types)
        self._trainable_base_dist = bool(trainable_base_dist)
        self._n_dims = int(n_dims)
        self._make_distribution = self._get_distribution_fn(n_dims, self._flow_types, trainable_base_dist)

    def __call__(self, t) -> FlowDistribution:
        return self._make_distribution(t)

    @property
    def flow_types(self):
        return self._flow_types

    @property
    def n_dims(self):
        return self._n_dims

    @property
    def trainable_base_dist(self):
        return self._trainable_base_dist

    @staticmethod
    def _get_distribution_fn(n_dims, flow_types, trainable_base_dist):
        return lambda t: FlowDistribution(t, n_dims, flow_types, trainable_base_dist)

    def get_total_param_size(self):
        """Width of ``t``: flow blocks + ``2*n_dims`` for a trainable base."""
        return ops.total_param_size(self._flow_types, self._n_dims, self._trainable_base_dist)

    # --- training hooks (BaseEstimator.fit dispatches through the layer) ---------
    def trainable_parameters(self, device) -> list:
        """The layer's own trainable tensors: none (every flow parameter is a column of t)."""
        return []

    def train_log_prob(self, y, t) -> torch.Tensor:
        """Differentiable ``log_prob(y | t)`` of a training step (fused forward / backward)."""
        return ops.log_prob(y, t, self._flow_types, self._n_dims, self._trainable_base_dist)

    def finish_training(self) -> None:
        pass

    def posterior_lse(self, y, t_draws, y_mean=None, y_std=None, **want):
        """``logsumexp_s(log_pdf(y_b | t_draws[s, b])) - log S`` per sample, fused
        (``BayesianNNEstimator.py:65-76``); ``want`` as for :func:`ops.posterior_lse`."""
        return ops.posterior_lse(y, t_draws, self._flow_types, self._n_dims, self._trainable_base_dist, y_mean,
                                 y_std, **want)

    @staticmethod
    def _get_bijector(t, flow_types, n_dims):
        """Chain of flows; blocks are split in REVERSED ``flow_types`` order and
        ``bijectors[0]`` is the last flow type (``DistributionLayers.py:267-278``).  As TF's
        slices are copies, the flows own a snapshot of ``t`` taken here (one device pass,
        ``flows.snapshot_rows``): later writes to ``t`` do not reach them."""
        flow_types = list(reversed(list(flow_types)))
        param_sizes = [FLOWS[flow_type].get_param_size(n_dims) for flow_type in flow_types]
        assert sum(param_sizes) == _shape(t)[-1]
        t = snapshot_rows(t)
        chain = []
        begin = 0
        for size, flow_type in zip(param_sizes, flow_types):
            chain.append(FLOWS[flow_type](_cols(t, begin, begin + size), n_dims))
            begin += size
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.stride(-1) == 1 and len(chain) > 1:
            # the flows' own launches read contiguous copies of their blocks of the snapshot,
            # made in one pass on the first such call (normalizing_flows.SplitBlocks)
            group = SplitBlocks(t, param_sizes)
            for k, f in enumerate(chain):
                f._split = (group, k)
        return Chain(chain)

    @staticmethod
    def _get_base_dist(t, n_dims, trainable) -> MultivariateNormalDiag:
        return MultivariateNormalDiag(t, n_dims, trainable)


# ---------------------------------------------------------------------------
# Kernel mixture network (estimators/DistributionLayers.py:74-172)
# ---------------------------------------------------------------------------

def cosine_distances(a: np.ndarray) -> np.ndarray:
    """Pairwise ``1 - cos(a_i, a_j)`` (scikit-learn's ``cosine_distances``: rows normalised
    with zero norms left as they are, clipped to [0, 2], exact zeros on the diagonal)."""
    a = np.asarray(a, np.float64)
    n = np.linalg.norm(a, axis=1, keepdims=True)
    n[n == 0.0] = 1.0
    u = a / n
    dist = np.clip(1.0 - u @ u.T, 0.0, 2.0)
    np.fill_diagonal(dist, 0.0)
    return dist


def kmeans_centers(y: np.ndarray, k: int, seed: int = 22, n_iter: int = 100) -> np.ndarray:
    """``k`` cluster centres of ``y`` (n, d) by a small seeded k-means: k-means++ seeding and
    Lloyd iterations until the assignment stops changing.  Stands in for the reference's
    ``sklearn.cluster.KMeans(n_clusters=k).fit(y).cluster_centers_``
    (``DistributionLayers.py:162-164``); an empty cluster keeps its previous centre."""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    assert 1 <= k <= n, f"k-means needs 1 <= k <= {n} points, got k = {k}"
    rng = np.random.default_rng(seed)
    centers = np.empty((k, y.shape[1]), np.float64)
    centers[0] = y[rng.integers(n)]
    d2 = np.sum((y - centers[0]) ** 2, axis=1)
    for c in range(1, k):
        tot = d2.sum()
        idx = int(rng.choice(n, p=d2 / tot)) if tot > 0.0 else int(rng.integers(n))
        centers[c] = y[idx]
        d2 = np.minimum(d2, np.sum((y - centers[c]) ** 2, axis=1))
    assign = None
    for _ in range(n_iter):
        dist = ((y[:, None, :] - centers[None, :, :]) ** 2).sum(-1)
        new = np.argmin(dist, axis=1)
        if assign is not None and np.array_equal(new, assign):
            break
        assign = new
        for c in range(k):
            members = y[assign == c]
            if len(members):
                centers[c] = members.mean(axis=0)
    return centers


class KernelMixtureDistribution(_RowDensity):
    """``MixtureSameFamily(Categorical(logits=t), MultivariateNormalDiag(locs, scale_identity_
    multiplier=scales))`` of the reference (``DistributionLayers.py:118-133``), evaluated by
    the fused mixture kernel (``nfn_kernel_mixture_logprob_f32``)."""

    def __init__(self, t, locs, scales, n_dims: int):
        super().__init__(t, n_dims)
        self._locs = locs
        self._scales = scales

    def _forward(self, y, t, y_mean, y_std, **want):
        return ops.kernel_mixture_log_prob(y, t, self._locs, self._scales, y_mean, y_std, **want)

    def _diff(self, y, t, y_mean, y_std):
        return ops.kernel_mixture_log_prob_diff(y, t, self._locs, self._scales, y_mean, y_std)

    def _grad_inputs(self) -> tuple:
        return (self._scales,)


class GaussianKernelsLayer:
    """Turns a logit tensor ``t (..., n_centers * n_scales)`` into a mixture of Gaussian
    kernels at fixed centres (``estimators/DistributionLayers.py:74-172``; a Keras
    ``DistributionLambda`` there, a plain callable here).

    ``locs`` (M, d) is the ``n_centers`` centres repeated per scale (scale 0's block first),
    zeros until :meth:`set_center_points`; it is not trained.  The bandwidth of scale ``i`` is
    ``softplus(v[i]) + log(expm1(init_scales[i]))`` with ``v`` a trainable ``(n_scales,)``
    variable initialised to zeros.

    QUIRK kept from the reference: that formula is not a softplus-inverse parametrisation —
    at ``v = 0`` and ``init = 0.3`` it is ``0.6931 - 1.0502 = -0.3571``, a NEGATIVE scale.
    TFP's ``MultivariateNormalDiag`` evaluates it through ``log|s|`` and ``(./s)^2``, so the
    density is that of ``|s|``; the kernels do the same and the formula is not "fixed"."""

    def __init__(self, n_centers, n_dims, trainable_scale=True, init_scales=(0.3, 0.7)):
        self.n_centers = int(n_centers)
        self.n_scales = len(init_scales)
        self.n_dims = int(n_dims)
        self.trainable_scale = bool(trainable_scale)
        self.init_scales = tuple(float(s) for s in init_scales)
        self._offsets = torch.tensor([float(np.log(np.expm1(s))) for s in self.init_scales], dtype=torch.float32)
        self.v = torch.zeros((self.n_scales,), dtype=torch.float32)
        self.locs = np.zeros((self.n_scales * self.n_centers, self.n_dims), np.float32)
        self._locs_dev = None

    def get_total_param_size(self):
        return self.n_centers * self.n_scales

    def scales(self, device=None) -> torch.Tensor:
        """The (M,) bandwidths, differentiable in ``v`` (plain torch ops: the map from
        ``grad_scales`` to ``v`` — sigmoid, sum over each scale's block — is autograd's)."""
        dev = self.v.device if device is None else device
        s = torch.nn.functional.softplus(self.v.to(dev)) + self._offsets.to(dev)
        return s.repeat_interleave(self.n_centers)

    def _device_locs(self, dev) -> torch.Tensor:
        if self._locs_dev is None or self._locs_dev.device != dev:
            self._locs_dev = torch.as_tensor(self.locs, dtype=torch.float32, device=dev).contiguous()
        return self._locs_dev

    def __call__(self, t) -> KernelMixtureDistribution:
        assert _shape(t)[-1] == self.n_centers * self.n_scales  # DistributionLayers.py:120
        dev = ops._device()
        return KernelMixtureDistribution(t, self._device_locs(dev), self.scales(dev), self.n_dims)

    # --- training hooks (BaseEstimator.fit) -------------------------------------
    def trainable_parameters(self, device) -> list:
        """Moves ``v`` to ``device`` as a leaf that requires grad and returns the layer's
        trainable tensors (none with ``trainable_scale=False``)."""
        self.v = self.v.detach().to(device).requires_grad_(self.trainable_scale)
        self._offsets = self._offsets.to(device)
        return [self.v] if self.trainable_scale else []

    def train_log_prob(self, y, t) -> torch.Tensor:
        return ops.kernel_mixture_log_prob_diff(y, t, self._device_locs(t.device), self.scales(t.device))

    def finish_training(self) -> None:
        self.v = self.v.detach()

    def posterior_lse(self, y, t_draws, y_mean=None, y_std=None, **want):
        """``logsumexp_s(log_pdf(y_b | t_draws[s, b])) - log S`` per sample, fused
        (``BayesianNNEstimator.py:65-76``); ``want`` as for :func:`ops.posterior_lse`."""
        dev = ops._device()
        with torch.no_grad():
            return ops.posterior_lse_kernel_mixture(y, t_draws, self._device_locs(dev), self.scales(dev), y_mean,
                                                    y_std, **want)

    def set_center_points(self, y, seed: int = 22):
        """``DistributionLayers.py:135-172``: ``n_edge = min(2 d, n_centers // 2)`` centres on
        the data's rim — among the ``2 n_edge`` points farthest from the mean, picked greedily
        so that the smallest cosine distance to those already picked is largest — the picked
        points removed from the data, k-means for the other ``n_centers - n_edge`` centres
        (:func:`kmeans_centers`, seeded), and the centres tiled once per scale."""
        y = np.asarray(y, np.float64)
        assert y.ndim == 2 and y.shape[1] == self.n_dims
        n_edge_points = min(2 * y.shape[1], self.n_centers // 2)
        parts = []
        if n_edge_points > 0:
            farthest_idx = np.argsort(np.linalg.norm(y - y.mean(axis=0), axis=1))[-2 * n_edge_points:]
            y_farthest = y[farthest_idx]
            dists = cosine_distances(y_farthest)
            selected = [0]
            for _ in range(1, n_edge_points):
                selected.append(int(np.argsort(np.min(dists[:, selected], axis=1), axis=0)[-1]))
            parts.append(y_farthest[selected])
            y = np.delete(y, farthest_idx[selected], axis=0)
        k = self.n_centers - n_edge_points
        if k > 0:
            parts.append(kmeans_centers(y, k, seed=seed))
        centers = np.concatenate(parts, axis=0)
        self.locs = np.float32(np.concatenate([centers] * self.n_scales, axis=0))
        self._locs_dev = None


# ---------------------------------------------------------------------------
# Mixture density network (estimators/DistributionLayers.py:174-212)
# ---------------------------------------------------------------------------

class GaussianMixtureDistribution(_RowDensity):
    """``Mixture(Categorical(logits), K x MultivariateNormalDiag(loc_k, softplus(0.05 raw_k +
    log(expm1(1)))))`` of the reference (``DistributionLayers.py:196-212``), every parameter
    read from the row ``t``, evaluated by the fused Gaussian-mixture kernel
    (``nfn_gaussian_mixture_logprob_f32``)."""

    def __init__(self, t, n_centers: int, n_dims: int):
        super().__init__(t, n_dims)
        self._n_centers = int(n_centers)

    def _forward(self, y, t, y_mean, y_std, **want):
        return ops.gaussian_mixture_log_prob(y, t, self._n_centers, self._n_dims, y_mean, y_std, **want)

    def _diff(self, y, t, y_mean, y_std):
        return ops.gaussian_mixture_log_prob_diff(y, t, self._n_centers, self._n_dims, y_mean, y_std)


class GaussianMixtureLayer:
    """Turns a parameter tensor ``t (..., n_centers * (2 * n_dims + 1))`` into a mixture of
    ``n_centers`` diagonal Gaussians whose locations, scales and mixture weights all come from
    ``t`` (``estimators/DistributionLayers.py:174-212``; a Keras ``DistributionLambda`` there,
    a plain callable here).  Row layout: ``[loc_0 | raw_0 | ... | loc_{K-1} | raw_{K-1} |
    logits]``.  The layer has no parameters of its own."""

    def __init__(self, n_centers, n_dims):
        self.n_centers = int(n_centers)
        self.n_dims = int(n_dims)

    def get_total_param_size(self):
        return self.n_centers + 2 * self.n_dims * self.n_centers

    def __call__(self, t) -> GaussianMixtureDistribution:
        # the reference's slices would give components of the wrong event size (a shape error)
        assert _shape(t)[-1] == self.get_total_param_size()
        return GaussianMixtureDistribution(t, self.n_centers, self.n_dims)

    # --- training hooks (BaseEstimator.fit) -------------------------------------
    def trainable_parameters(self, device) -> list:
        return []

    def train_log_prob(self, y, t) -> torch.Tensor:
        return ops.gaussian_mixture_log_prob_diff(y, t, self.n_centers, self.n_dims)

    def finish_training(self) -> None:
        pass

    def posterior_lse(self, y, t_draws, y_mean=None, y_std=None, **want):
        """``logsumexp_s(log_pdf(y_b | t_draws[s, b])) - log S`` per sample, fused
        (``BayesianNNEstimator.py:65-76``); ``want`` as for :func:`ops.posterior_lse`."""
        return ops.posterior_lse_gaussian_mixture(y, t_draws, self.n_centers, self.n_dims, y_mean, y_std, **want)
