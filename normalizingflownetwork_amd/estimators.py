"""Estimator surface around the flow hot path.

Mirrors ``estimators/BaseEstimator.py:43-86``, ``MaximumLikelihoodNNEstimator.py``,
``NormalizingFlowNetwork.py`` and ``BayesNormalizingFlowNetwork.py`` /
``BayesianNNEstimator.py:65-76`` for EVALUATION: ``log_pdf``, ``pdf``, ``score``.

The x -> t network (the reference's Keras Dense stack) is not on the hot path
(out of scope); it is a small torch MLP here, used only to
produce ``t``.  Everything from ``t`` to the density / score runs in the fused
HIP kernels: the y normalisation ``(y - mu)/sigma``, the whole flow chain, the
base density, the ``-sum(log sigma)`` correction and (for ``score``) the fp64
batch sum.  ``fit`` trains on the GPU: torch autograd through the MLP and the
fused backward kernel through the flow chain; the Bayesian
estimator's variational training (``fit(variational=True)``: weight draw, KL term and their
gradients) runs in the two fused mean-field kernels.

``KernelMixtureNetwork`` (``estimators/KernelMixtureNetwork.py``) shares all of it: ``fit``
dispatches through the density layer (its trainable tensors, its differentiable train-time
``log_prob``), so the same loop trains the flow chain or the kernel mixture.
``MixtureDensityNetwork`` (``estimators/MixtureDensityNetwork.py``) is the third such layer.

``BayesianNNEstimator`` holds the posterior machinery (weight draws, ``params_draws``,
``evaluate``, the chunked fused ``score``) for any of the three layers:
``BayesNormalizingFlowNetwork`` (which keeps its fused-Dense ``score``),
``BayesMixtureDensityNetwork`` and ``BayesKernelMixtureNetwork``.
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .distribution_layers import GaussianKernelsLayer, GaussianMixtureLayer, InverseNormalizingFlowLayer

_ACTIVATIONS = {
    "tanh": torch.tanh,
    "relu": torch.relu,
    "linear": lambda v: v,
    "sigmoid": torch.sigmoid,
    "elu": torch.nn.functional.elu,
}


class _MLP:
    """Dense stack x -> t (``MaximumLikelihoodNNEstimator.py:37-44``), Glorot-uniform
    weights and zero biases like Keras' ``Dense`` defaults."""

    def __init__(self, n_in: int, hidden_sizes: Sequence[int], n_out: int, activation: str, seed: int):
        assert type(hidden_sizes) in (tuple, list)
        assert activation in _ACTIVATIONS, f"unknown activation {activation!r}"
        g = torch.Generator().manual_seed(seed)
        sizes = [n_in] + list(hidden_sizes) + [n_out]
        self.weights, self.biases = [], []
        for a, b in zip(sizes[:-1], sizes[1:]):
            lim = float(np.sqrt(6.0 / (a + b)))
            self.weights.append((torch.rand((a, b), generator=g, dtype=torch.float32) * 2 - 1) * lim)
            self.biases.append(torch.zeros((b,), dtype=torch.float32))
        self.activation = activation
        self._device = None

    def to(self, device):
        if self._device != device:
            self.weights = [w.to(device) for w in self.weights]
            self.biases = [b.to(device) for b in self.biases]
            self._device = device
        return self

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        act = _ACTIVATIONS[self.activation]
        h = x
        n = len(self.weights)
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            h = h @ w + b
            if i < n - 1:
                h = act(h)
        return h

    def hidden(self, x: torch.Tensor) -> torch.Tensor:
        """Activations entering the linear output layer (the fused Dense path's input)."""
        act = _ACTIVATIONS[self.activation]
        h = x
        for w, b in zip(self.weights[:-1], self.biases[:-1]):
            h = act(h @ w + b)
        return h.contiguous()


class BaseEstimator:
    """Evaluation half of ``estimators/BaseEstimator.py``."""

    def __init__(self, dist_layer: InverseNormalizingFlowLayer, n_dims_x: Optional[int] = None,
                 hidden_sizes=(16, 16), activation="relu", random_seed=22, noise_reg=("fixed_rate", 0.0)):
        assert len(noise_reg) == 2
        self.dist_layer = dist_layer
        self.n_dims = dist_layer.n_dims
        self.hidden_sizes = tuple(hidden_sizes)
        self.activation = activation
        self.random_seed = random_seed
        self.noise_fn_type, self.noise_scale_factor = noise_reg
        self.x_noise_std = self.y_noise_std = 0.0  # set by fit (BaseEstimator.py:9-10, 33-41)
        self.x_mean = self.x_std = None
        self.y_mean = np.zeros((self.n_dims,), np.float32)
        self.y_std = np.ones((self.n_dims,), np.float32)
        self._mlp = None
        # fit: the output Dense layer fused into the chain kernels (forward + backward)
        # when its shapes allow; False trains through the materialised t instead
        self.fused_dense = True
        self.last_score_nonfinite = 0
        if n_dims_x is not None:
            self._build(n_dims_x)

    # --- x -> t -----------------------------------------------------------------
    def _build(self, n_dims_x: int):
        self._mlp = _MLP(n_dims_x, self.hidden_sizes, self.dist_layer.get_total_param_size(), self.activation,
                         self.random_seed)
        if self.x_mean is None:
            self.x_mean = np.zeros((n_dims_x,), np.float32)
            self.x_std = np.ones((n_dims_x,), np.float32)

    def _assign_data_normalization(self, x, y):
        """``BaseEstimator.py:49-53``."""
        x = np.asarray(x, np.float32)
        y = np.asarray(y, np.float32)
        self.x_mean = np.mean(x, axis=0, dtype=np.float32)
        self.y_mean = np.mean(y, axis=0, dtype=np.float32)
        self.x_std = np.std(x, axis=0, dtype=np.float32)
        self.y_std = np.std(y, axis=0, dtype=np.float32)

    def set_data_normalization(self, x, y):
        self._assign_data_normalization(x, y)

    def params(self, x) -> torch.Tensor:
        """``t = MLP((x - mu_x)/(sigma_x + 1e-8))`` (``MaximumLikelihoodNNEstimator.py:40-43``)."""
        x = ops.as_device_f32(x)
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        if self._mlp is None:
            self._build(int(x.shape[-1]))
        dev = x.device
        self._mlp.to(dev)
        xm = torch.as_tensor(self.x_mean, dtype=torch.float32, device=dev)
        xs = torch.as_tensor(self.x_std, dtype=torch.float32, device=dev)
        return self._mlp((x - xm) / (xs + 1e-8)).contiguous()

    def __call__(self, x):
        return self.dist_layer(self.params(x))

    def _fused_dense_inputs(self, x):
        """``(h, W, b)`` of the output Dense layer when the fused Dense->chain kernel takes
        the shapes (evaluation only: no autograd through it), else None."""
        if not isinstance(self.dist_layer, InverseNormalizingFlowLayer):
            return None  # the fused Dense kernels evaluate a flow chain
        if torch.is_grad_enabled() and any(w.requires_grad for w in (self._mlp.weights if self._mlp else [])):
            return None
        x = ops.as_device_f32(x)
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        if self._mlp is None:
            self._build(int(x.shape[-1]))
        self._mlp.to(x.device)
        W, b = self._mlp.weights[-1], self._mlp.biases[-1]
        if not ops.dense_fusable(int(W.shape[0]), int(W.shape[1]), self.n_dims) or len(self._mlp.weights) < 2:
            return None
        xm = torch.as_tensor(self.x_mean, dtype=torch.float32, device=x.device)
        xs = torch.as_tensor(self.x_std, dtype=torch.float32, device=x.device)
        return self._mlp.hidden((x - xm) / (xs + 1e-8)), W, b

    def call(self, x, training=False):
        return self(x)

    # --- evaluation ---------------------------------------------------------------
    def log_pdf(self, x, y):
        """``BaseEstimator.py:77-86``: ``log_prob((y-mu)/sigma) - sum(log sigma)``."""
        x = np.asarray(x, np.float32) if not isinstance(x, torch.Tensor) else x
        y = np.asarray(y, np.float32) if not isinstance(y, torch.Tensor) else y
        assert tuple(x.shape) == tuple(y.shape)
        fused = self._fused_dense_inputs(x)
        if fused is not None:  # output Dense layer fused into the chain kernel
            dl = self.dist_layer
            lp, _ = ops.chain_log_prob_dense(y, *fused, dl.flow_types, self.n_dims, dl.trainable_base_dist,
                                             self.y_mean, self.y_std)
            return lp
        output = self(x)
        assert output.event_shape == y.shape[-1]
        return output.log_prob(y, self.y_mean, self.y_std)

    def pdf(self, x, y):
        """``BaseEstimator.py:71-75``: ``prob(y_circ) / prod(sigma)`` = ``exp(log_pdf)``."""
        return torch.exp(self.log_pdf(x, y))

    def score(self, x_data, y_data) -> float:
        """``BaseEstimator.py:43-47``: mean log-likelihood, reduced on the device in fp64."""
        x_data = np.asarray(x_data, np.float32) if not isinstance(x_data, torch.Tensor) else x_data
        y_data = np.asarray(y_data, np.float32) if not isinstance(y_data, torch.Tensor) else y_data
        fused = self._fused_dense_inputs(x_data)
        if fused is not None:  # output Dense layer fused into the chain kernel
            dl = self.dist_layer
            _, s, nf = ops.chain_log_prob_dense(y_data, *fused, dl.flow_types, self.n_dims, dl.trainable_base_dist,
                                                self.y_mean, self.y_std, want_values=False, want_nonfinite=True)
        else:
            output = self(x_data)
            s, nf = output.log_prob_sum(y_data, self.y_mean, self.y_std, want_nonfinite=True)
        return self._finish_score(s, nf, int(y_data.shape[0]))

    def _finish_score(self, s: torch.Tensor, nf: torch.Tensor, n: int) -> float:
        """Mean from the device fp64 sum.  Non-finite log-densities propagate into the
        mean exactly as in the reference's ``.mean()`` (``BaseEstimator.py:47``); their
        count (kept as ``last_score_nonfinite``) is reported with a ``RuntimeWarning``
        instead of passing silently."""
        vals = torch.cat([s.reshape(1), nf.reshape(1)]).cpu().tolist()
        self.last_score_nonfinite = int(vals[1])
        if self.last_score_nonfinite:
            import warnings

            warnings.warn(f"score: {self.last_score_nonfinite} of {n} log-densities are not finite",
                          RuntimeWarning, stacklevel=3)
        return vals[0] / n

    def _get_input_model(self):
        """``BaseEstimator.py:61-69``: ``y -> (y - mu_y) / sigma_y`` followed by Keras
        ``GaussianNoise(y_noise_std)``, which adds noise only when called with
        ``training=True``.  Returns ``input_model(y, training=False)`` (a device tensor)."""
        gen = {}

        def input_model(y, training=False):
            y = ops.as_device_f32(y)
            ym = torch.as_tensor(self.y_mean, dtype=torch.float32, device=y.device)
            ys = torch.as_tensor(self.y_std, dtype=torch.float32, device=y.device)
            yc = (y - ym) / ys
            if training and self.y_noise_std > 0.0:
                if "g" not in gen:
                    gen["g"] = torch.Generator(device=y.device)
                    gen["g"].manual_seed(int(self.random_seed) + 7)
                yc = yc + self.y_noise_std * torch.randn(yc.shape, generator=gen["g"], device=y.device,
                                                         dtype=yc.dtype)
            return yc

        return input_model

    def _get_neg_log_likelihood(self):
        """``BaseEstimator.py:55-59``: the compiled loss, ``nll(y, p_y) = -p_y.log_prob(
        input_model(y)) + sum(log sigma_y)`` per sample (noise off: evaluation)."""
        input_model = self._get_input_model()
        log_sy = float(np.sum(np.log(np.asarray(self.y_std, np.float64))))
        return lambda y, p_y: -p_y.log_prob(input_model(y)) + log_sy

    def evaluate(self, x, y, batch_size=None, verbose=0, **kwargs) -> float:
        """Keras ``Model.evaluate`` of the compiled loss (``MaximumLikelihoodNNEstimator.py:33-35``):
        the sample mean of ``_get_neg_log_likelihood()(y, self(x))`` with noise off.  The
        per-batch means Keras averages (weighted by batch size) equal this one mean, so the
        data runs as one batch: the MLP in torch, ``log_prob`` in the fused chain kernel on
        the materialised ``t`` (``score`` takes the fused Dense -> chain path: the reference's
        ``score == -evaluate`` tests compare the two)."""
        x = np.asarray(x, np.float32) if not isinstance(x, torch.Tensor) else x
        y = np.asarray(y, np.float32) if not isinstance(y, torch.Tensor) else y
        with torch.no_grad():
            nll = self._get_neg_log_likelihood()(y, self.call(x, training=False))
        return float(nll.double().mean().item())

    def _assign_noise_regularisation(self, n_dims: int, n_datapoints: int):
        """``BaseEstimator.py:33-41``."""
        assert self.noise_fn_type in ["rule_of_thumb", "fixed_rate"]
        if self.noise_fn_type == "rule_of_thumb":
            std = self.noise_scale_factor * (n_datapoints + 1) ** (-1 / (4 + n_dims))
        else:
            std = self.noise_scale_factor
        self.x_noise_std = self.y_noise_std = float(std)

    def fit(self, x, y, batch_size=None, epochs=None, verbose=1, shuffle=True, use_graph=True, **kwargs):
        """Maximum-likelihood training on the GPU: ``BaseEstimator.fit`` (``BaseEstimator.py:19-31``)
        with the model compiled as in ``MaximumLikelihoodNNEstimator.py:33-35`` —
        Adam(learning_rate), loss = mean over the batch of ``-log_prob(y_circ + noise | t)
        + sum(log y_std)`` (``BaseEstimator.py:55-67``), Keras defaults ``batch_size=32``,
        ``epochs=1``, per-epoch shuffling, GaussianNoise on the normalised x and y while
        training, and TerminateOnNaN.  ``t = MLP(x)`` runs in torch; ``log_prob`` and its
        gradient w.r.t. ``t`` run in the fused HIP kernels (``nfn_chain_logprob_f32`` /
        ``nfn_chain_logprob_grad_f32``).

        At the reference's batch sizes a training step is a few dozen tiny launches, so with
        ``use_graph`` the full-batch step (gather, normalisation, MLP, fused log_prob forward
        and backward, Adam) is captured once into a HIP graph and replayed: per step only the
        batch indices and the noise draws (if any) are written into the graph's static inputs
        — the same generator calls in the same order as the eager loop, so both paths train
        identically.  A final partial batch runs eagerly.  Returns ``{"loss": [per-epoch
        mean loss]}``."""
        x = np.asarray(x, np.float32)
        y = np.asarray(y, np.float32)
        assert len(x.shape) == len(y.shape) == 2, "Please pass a matrix not a vector"
        self._assign_data_normalization(x, y)
        self._assign_noise_regularisation(n_dims=x.shape[1] + y.shape[1], n_datapoints=x.shape[0])
        if self._mlp is None:
            self._build(int(x.shape[1]))
        dev = ops._device()
        self._mlp.to(dev)
        params = self._fit_begin(dev)
        n_eps = self._fit_draw_size()
        lr = getattr(self, "learning_rate", 3e-3)
        dl = self.dist_layer
        # the layer's own trainable tensors (the kernel mixture's bandwidth variable; a flow
        # layer has none: everything it evaluates comes out of the MLP)
        layer_params = dl.trainable_parameters(dev)
        # Keras Adam defaults; capturable: the step counts and bias corrections live on the
        # device, so the same optimizer runs eagerly and inside the graph
        opt = torch.optim.Adam(params + layer_params, lr=lr, betas=(0.9, 0.999), eps=1e-7, capturable=True)
        P = dl.get_total_param_size()
        # the output Dense layer can be fused into the flow chain's kernels only
        fused_dense = (isinstance(dl, InverseNormalizingFlowLayer) and len(self._mlp.weights) > 1
                       and self.fused_dense
                       and ops.dense_fusable(int(self._mlp.weights[-1].shape[0]), P, self.n_dims))
        batch_size = 32 if batch_size is None else int(batch_size)
        epochs = 1 if epochs is None else int(epochs)
        X = torch.from_numpy(x).to(dev)
        Y = torch.from_numpy(y).to(dev)
        xm, xs = (torch.as_tensor(v, dtype=torch.float32, device=dev) for v in (self.x_mean, self.x_std))
        ym, ys = (torch.as_tensor(v, dtype=torch.float32, device=dev) for v in (self.y_mean, self.y_std))
        sum_log_ys = torch.log(ys).sum()
        gen = torch.Generator(device=dev).manual_seed(int(self.random_seed))
        n = X.shape[0]
        acc = torch.zeros((), dtype=torch.float64, device=dev)
        acc_pen = torch.zeros((), dtype=torch.float64, device=dev) if n_eps is not None else None

        def step(idx, nx, ny, eps):
            """One training step on the rows ``idx`` with the noise draws ``nx`` / ``ny`` and the
            weight draw ``eps``."""
            xn = (X[idx] - xm) / (xs + 1e-8)
            if nx is not None:
                xn = xn + self.x_noise_std * nx
            yc = (Y[idx] - ym) / ys
            if ny is not None:
                yc = yc + self.y_noise_std * ny
            mlp, penalty = self._fit_network(eps)
            if fused_dense:  # output layer fused into the chain, forward and backward
                lp = ops.log_prob_dense(yc, mlp.hidden(xn), mlp.weights[-1], mlp.biases[-1],
                                        dl.flow_types, self.n_dims, dl.trainable_base_dist)
            else:
                t = mlp(xn)
                lp = dl.train_log_prob(yc, t)  # the layer's differentiable fused log_prob
            loss = -lp.mean() + sum_log_ys
            if penalty is not None:
                loss = loss + penalty
                acc_pen.add_(penalty.detach().double() * idx.numel())
            loss.backward()
            opt.step()
            acc.add_(loss.detach().double() * idx.numel())

        def draws(rows):
            """The step's normal draws, in the fixed order the replay refills them."""
            nx = torch.randn((rows, X.shape[1]), generator=gen, device=dev) if self.x_noise_std > 0 else None
            ny = torch.randn((rows, Y.shape[1]), generator=gen, device=dev) if self.y_noise_std > 0 else None
            eps = torch.randn((n_eps,), generator=gen, device=dev) if n_eps else None
            return nx, ny, eps

        graph = None  # (graph, static idx, static draws (x noise, y noise, eps), its pinned workspaces)
        warm = 3  # eager steps before the capture (optimizer state, allocator pools)
        steps_done = 0
        history = {"loss": []} if acc_pen is None else {"loss": [], "nll": [], "kl": []}
        try:
            for _ in range(epochs):
                perm = torch.randperm(n, generator=gen, device=dev) if shuffle else torch.arange(n, device=dev)
                acc.zero_()
                if acc_pen is not None:
                    acc_pen.zero_()
                for i in range(0, n, batch_size):
                    idx = perm[i:i + batch_size]
                    full = idx.numel() == batch_size
                    if use_graph and full and graph is not None:
                        g_, sidx, static, _ = graph
                        sidx.copy_(idx)
                        for buf in static:
                            if buf is not None:
                                buf.normal_(generator=gen)
                        g_.replay()
                        continue
                    noise = draws(idx.numel())
                    if use_graph and full and steps_done >= warm:
                        # capture the full-batch step (the capture itself executes nothing:
                        # this batch then runs as the graph's first replay)
                        sidx = idx.clone()
                        opt.zero_grad(set_to_none=True)
                        side = torch.cuda.Stream(device=dev)
                        side.wait_stream(torch.cuda.current_stream(dev))
                        g_ = torch.cuda.CUDAGraph()
                        mark = ops.graph_pin_mark()
                        with torch.cuda.stream(side):
                            with torch.cuda.graph(g_, stream=side):
                                step(sidx, *noise)
                        torch.cuda.current_stream(dev).wait_stream(side)
                        # the workspaces the capture pinned live exactly as long as this graph
                        graph = (g_, sidx, noise, ops.take_graph_workspaces(side, mark))
                        g_.replay()
                        continue
                    opt.zero_grad(set_to_none=True)
                    if use_graph and steps_done < warm:
                        side = torch.cuda.Stream(device=dev)  # warm-up on a side stream (capture rules)
                        side.wait_stream(torch.cuda.current_stream(dev))
                        with torch.cuda.stream(side):
                            step(idx, *noise)
                        torch.cuda.current_stream(dev).wait_stream(side)
                    else:
                        step(idx, *noise)
                    steps_done += 1
                ep_loss = float(acc.item()) / n
                history["loss"].append(ep_loss)
                if acc_pen is not None:  # loss = nll + kl, the weighted KL term as Keras adds it
                    ep_kl = float(acc_pen.item()) / n
                    history["kl"].append(ep_kl)
                    history["nll"].append(ep_loss - ep_kl)
                if verbose:
                    print(f"epoch {len(history['loss'])}/{epochs} loss {ep_loss:.6f}", flush=True)
                if not np.isfinite(ep_loss):  # tf.keras.callbacks.TerminateOnNaN
                    break
        finally:
            self._fit_end()
            dl.finish_training()
        return history

    # --- what a training step trains: the Bayesian estimator's variational fit overrides these
    def _fit_begin(self, dev) -> list:
        """The network's trainable tensors (leaves on ``dev``) for the optimizer."""
        params = [p.detach().requires_grad_(True) for p in self._mlp.weights + self._mlp.biases]
        nw = len(self._mlp.weights)
        self._mlp.weights, self._mlp.biases = params[:nw], params[nw:]
        return params

    def _fit_draw_size(self) -> Optional[int]:
        """Length of the N(0, 1) weight draw a step takes after its noise draws; None: the step
        has no weight draw and no penalty term (0: a penalty, but nothing to draw)."""
        return None

    def _fit_network(self, eps):
        """``(network, penalty)`` of one step: the x -> t network to run and the term its loss
        adds to the batch-mean NLL (None: nothing)."""
        return self._mlp, None

    def _fit_end(self):
        """Leave the trained values in the estimator."""
        self._mlp.weights = [p.detach() for p in self._mlp.weights]
        self._mlp.biases = [p.detach() for p in self._mlp.biases]


class NormalizingFlowNetwork(BaseEstimator):
    """``estimators/NormalizingFlowNetwork.py:9-19``: ``n_flows`` radial flows by
    default.  ``flow_types`` (a compatible superset) picks any chain, e.g. the
    planar/radial chains of the benchmark configs."""

    def __init__(self, n_dims, n_flows=10, trainable_base_dist=True, flow_types=None, hidden_sizes=(16, 16),
                 noise_reg=("fixed_rate", 0.0), learning_rate=3e-3, activation="relu", random_seed=22,
                 n_dims_x=None):
        flow_types = tuple(flow_types) if flow_types is not None else ("radial",) * n_flows
        dist_layer = InverseNormalizingFlowLayer(flow_types=flow_types, n_dims=n_dims,
                                                 trainable_base_dist=trainable_base_dist)
        self.learning_rate = learning_rate
        super().__init__(dist_layer, n_dims_x=n_dims_x, hidden_sizes=hidden_sizes, activation=activation,
                         random_seed=random_seed, noise_reg=noise_reg)

    @staticmethod
    def build_function(n_dims=1, n_flows=3, hidden_sizes=(16, 16), trainable_base_dist=True,
                       noise_reg=("fixed_rate", 0.0), learning_rate=3e-3, activation="tanh"):
        return NormalizingFlowNetwork(n_dims=n_dims, n_flows=n_flows, hidden_sizes=hidden_sizes,
                                      trainable_base_dist=trainable_base_dist, noise_reg=noise_reg,
                                      learning_rate=learning_rate, activation=activation)


class KernelMixtureNetwork(BaseEstimator):
    """``estimators/KernelMixtureNetwork.py``: an MLP whose output is the logit row of a
    mixture of Gaussian kernels at centres fixed from the training targets
    (``GaussianKernelsLayer``), trained by maximum likelihood together with the layer's
    bandwidth variable.  ``log_prob`` and its gradient run in the fused mixture kernels
    (``nfn_kernel_mixture_logprob_f32`` / ``nfn_kernel_mixture_logprob_grad_f32``)."""

    def __init__(self, n_dims, n_centers=50, hidden_sizes=(16, 16), noise_reg=("fixed_rate", 0.0),
                 learning_rate=3e-3, activation="relu", random_seed=22, n_dims_x=None):
        dist_layer = GaussianKernelsLayer(n_centers=n_centers, n_dims=n_dims, trainable_scale=True)
        self.learning_rate = learning_rate
        super().__init__(dist_layer, n_dims_x=n_dims_x, hidden_sizes=hidden_sizes, activation=activation,
                         random_seed=random_seed, noise_reg=noise_reg)

    @staticmethod
    def build_function(n_dims=1, n_centers=30, hidden_sizes=(16, 16), noise_reg=("fixed_rate", 0.0),
                       learning_rate=2e-3, activation="relu"):
        return KernelMixtureNetwork(n_dims=n_dims, n_centers=n_centers, hidden_sizes=hidden_sizes,
                                    noise_reg=noise_reg, learning_rate=learning_rate, activation=activation)

    def fit(self, x, y, batch_size=None, epochs=None, verbose=1, **kwargs):
        """``KernelMixtureNetwork.py:35-39``: the kernel centres are set from the normalised
        targets, then the MLP and the bandwidth variable train as in ``BaseEstimator.fit``."""
        y = np.asarray(y, np.float32)
        y_mean = np.mean(y, axis=0, dtype=np.float32)
        y_std = np.std(y, axis=0, dtype=np.float32)
        self.dist_layer.set_center_points((y - y_mean) / y_std, seed=int(self.random_seed))
        return super().fit(x, y, batch_size=batch_size, epochs=epochs, verbose=verbose, **kwargs)


class MixtureDensityNetwork(BaseEstimator):
    """``estimators/MixtureDensityNetwork.py``: an MLP whose output row holds the locations,
    scales and mixture logits of ``n_centers`` diagonal Gaussians (``GaussianMixtureLayer``),
    trained by maximum likelihood.  ``log_prob`` and its gradient run in the fused
    Gaussian-mixture kernels (``nfn_gaussian_mixture_logprob_f32`` /
    ``nfn_gaussian_mixture_logprob_grad_f32``)."""

    def __init__(self, n_dims, n_centers, hidden_sizes=(16, 16), noise_reg=("fixed_rate", 0.0),
                 learning_rate=3e-3, activation="relu", random_seed=22, n_dims_x=None):
        dist_layer = GaussianMixtureLayer(n_centers=n_centers, n_dims=n_dims)
        self.learning_rate = learning_rate
        super().__init__(dist_layer, n_dims_x=n_dims_x, hidden_sizes=hidden_sizes, activation=activation,
                         random_seed=random_seed, noise_reg=noise_reg)

    @staticmethod
    def build_function(n_dims=1, n_centers=5, hidden_sizes=(16, 16), noise_reg=("fixed_rate", 0.0),
                       learning_rate=2e-3, activation="relu"):
        return MixtureDensityNetwork(n_dims=n_dims, n_centers=n_centers, hidden_sizes=hidden_sizes,
                                     noise_reg=noise_reg, learning_rate=learning_rate, activation=activation)


def mean_field_scale(rho: torch.Tensor) -> torch.Tensor:
    """Scale of the mean-field posterior over every DenseVariational weight:
    ``1e-3 + softplus(log(expm1(1)) + 0.05 * rho)`` (``MeanFieldLayer``,
    ``DistributionLayers.py:45-55``)."""
    return 1e-3 + torch.nn.functional.softplus(float(np.log(np.expm1(1.0))) + 0.05 * rho)


# score: the (S, rows, P) draws of one chunk stay at or under this many bytes (a fixed cap, not
# a tuned number: S = 50 draws of a P = 100 row are 20 KB per sample)
POSTERIOR_CHUNK_BYTES = 256 << 20


class BayesianNNEstimator(BaseEstimator):
    """Posterior-scoring half of ``estimators/BayesianNNEstimator.py`` for any density layer
    (``dist_layer``: a flow chain, the Gaussian mixture or the kernel mixture).  Every layer
    is a ``DenseVariational`` whose weights
    (kernel and bias) have a mean-field Gaussian posterior held as one variable vector
    ``[loc | rho]`` initialised N(0, 0.05) (Keras ``"normal"``; ``BayesianNNEstimator.py:92-107``,
    ``DistributionLayers.py:17-55``): a draw is ``loc + (1e-3 + softplus(log(e-1) + 0.05 rho))
    * eps``, one weight sample per layer per draw shared by the batch (``:122-145``); in
    ``map_mode`` the variable holds ``loc`` only and the weights ARE ``loc``.  ``score``
    forms ``t`` of the S draws with one batched GEMM and evaluates
    ``logsumexp_s(log_pdf) - log S`` per sample in ONE fused kernel per row chunk (the
    layer's ``posterior_lse``) instead of S model re-runs.
    ``fit`` trains the posterior means by maximum likelihood; ``fit(variational=True)``
    trains the reference's objective, mean NLL of one weight draw per step plus
    ``kl_weight_scale * KL(q || p)``, over means, scales and (``trainable_prior``) the prior
    means, the draw, the KL and their gradients in the two fused mean-field kernels
    (``nfn_mean_field_draw_kl_f32`` / ``nfn_mean_field_draw_kl_grad_f32``)."""

    def __init__(self, dist_layer, kl_weight_scale, kl_use_exact=True, hidden_sizes=(10,), activation="tanh",
                 learning_rate=3e-2, noise_reg=("fixed_rate", 0.0), trainable_prior=False, map_mode=False,
                 prior_scale=1.0, random_seed=22, n_dims_x=None):
        assert kl_weight_scale <= 1.0  # BayesianNNEstimator.py:120
        self.map_mode = map_mode
        self.prior_scale = prior_scale
        self.trainable_prior = trainable_prior
        self.kl_use_exact = kl_use_exact
        self.kl_weight_scale = kl_weight_scale
        self.learning_rate = learning_rate  # BayesianNNEstimator.py:61-63 (Adam(learning_rate))
        self._post_rho = None
        self._prior_loc = None  # flat prior means of every weight, set by a variational fit (None: zeros)
        self._vi = None         # the flat variational variables while fit(variational=True) runs
        super().__init__(dist_layer, n_dims_x=n_dims_x, hidden_sizes=hidden_sizes, activation=activation,
                         random_seed=random_seed, noise_reg=noise_reg)
        self._draw_gen = None

    def _build(self, n_dims_x: int):
        """Shapes from the Dense stack; the posterior variables replace its weights: the
        means ``loc`` live in ``self._mlp`` (so ``params`` is the posterior-mean network),
        the ``rho`` in ``self._post_rho`` (None in map mode)."""
        super()._build(n_dims_x)
        g = torch.Generator().manual_seed(int(self.random_seed) + 1)
        rhos = []
        for w, b in zip(self._mlp.weights, self._mlp.biases):
            size = w.numel() + b.numel()  # DenseVariational: kernel (in x units) then bias
            v = 0.05 * torch.randn((size if self.map_mode else 2 * size,), generator=g, dtype=torch.float32)
            w.copy_(v[:w.numel()].reshape(w.shape))
            b.copy_(v[w.numel():size])
            if not self.map_mode:
                rhos.append((v[size:size + w.numel()].reshape(w.shape).clone(), v[size + w.numel():].clone()))
        self._post_rho = None if self.map_mode else rhos

    def posterior_scales(self, device=None):
        """Per layer ``(scale_W, scale_b)`` of the mean-field posterior (None in map mode)."""
        if self._post_rho is None:
            return None
        return [(mean_field_scale(rw).to(device), mean_field_scale(rb).to(device)) for rw, rb in self._post_rho]

    # --- variational training ------------------------------------------------------------
    def _layer_sizes(self) -> list:
        """Per layer ``kernel.numel(), bias.numel()`` in the flat vector's order."""
        return [n for w, b in zip(self._mlp.weights, self._mlp.biases) for n in (w.numel(), b.numel())]

    @staticmethod
    def _flatten(pairs, dev) -> torch.Tensor:
        """Per-layer ``(kernel, bias)`` pairs as ONE flat vector, each layer as kernel (in, out)
        row-major then bias: the order TFP's ``DenseVariational`` splits its variable."""
        return torch.cat([t.detach().to(dev).reshape(-1) for pair in pairs for t in pair])

    def _unflatten(self, flat: torch.Tensor):
        """``(kernels, biases)`` as contiguous views of ``flat`` (one split, so one backward node)."""
        parts = flat.split(self._layer_sizes())
        kernels = [p.view(w.shape) for p, w in zip(parts[0::2], self._mlp.weights)]
        return kernels, list(parts[1::2])

    def _posterior_flat(self, dev):
        """``(loc, rho | None, prior_loc | None)`` of the current posterior as flat vectors."""
        self._mlp.to(dev)
        loc = self._flatten(zip(self._mlp.weights, self._mlp.biases), dev)
        rho = None if self._post_rho is None else self._flatten(self._post_rho, dev)
        prior = None if self._prior_loc is None else self._prior_loc.detach().to(dev).clone()
        return loc, rho, prior

    def fit(self, x, y, batch_size=None, epochs=None, verbose=1, variational=False, **kwargs):
        """``BaseEstimator.fit``.  By default the posterior means train by maximum likelihood.
        ``variational=True`` trains the reference's compiled model (``BayesianNNEstimator.py:
        42-63, 109-146``): per step ONE ``eps ~ N(0, 1)`` for all weights (after the noise draws,
        from the same generator), the draw ``w = loc + s * eps`` and KL(q || p) in one fused
        launch (``ops.mean_field_draw_kl_diff``; backward: one more), the layers' ``W``, ``b`` as
        views of ``w``, and ``loss = mean NLL + kl_weight_scale * KL`` — Keras adds each layer's
        ``kl_weight * KL`` to the batch-mean loss, and summing the layers first is the same
        number.  ``kl_use_exact``, ``prior_scale``, ``trainable_prior`` and ``map_mode`` act as
        in the reference.  One Adam covers ``loc``, ``rho`` (not in map mode), the prior means
        (``trainable_prior``) and the density layer's own tensors; the step replays from the same
        HIP graph, ``eps`` refilled in place.  ``history`` then also holds ``"nll"`` and ``"kl"``
        (the weighted term), ``"loss"`` being their sum."""
        self._vi = {} if variational else None
        try:
            return super().fit(x, y, batch_size=batch_size, epochs=epochs, verbose=verbose, **kwargs)
        finally:
            self._vi = None

    def _fit_begin(self, dev) -> list:
        if self._vi is None:
            return super()._fit_begin(dev)
        loc, rho, prior = self._posterior_flat(dev)
        if prior is None and self.trainable_prior:
            prior = torch.zeros_like(loc)
        train = [loc] + ([] if rho is None else [rho]) + ([prior] if self.trainable_prior else [])
        for p in train:
            p.requires_grad_(True)
        self._vi.update(loc=loc, rho=rho, prior=prior)
        return train

    def _fit_draw_size(self) -> Optional[int]:
        if self._vi is None:
            return None
        return 0 if self._vi["rho"] is None else int(self._vi["loc"].numel())

    def _fit_network(self, eps):
        if self._vi is None:
            return super()._fit_network(eps)
        v = self._vi
        w, kl = ops.mean_field_draw_kl_diff(v["loc"], v["rho"], eps, v["prior"], self.prior_scale, self.kl_use_exact)
        net = _MLP.__new__(_MLP)  # this step's network: the drawn weights in the Dense stack's shapes
        net.activation = self.activation
        net.weights, net.biases = self._unflatten(w)
        return net, self.kl_weight_scale * kl

    def _fit_end(self):
        if not self._vi:  # maximum likelihood, or a variational fit that failed before it began
            return super()._fit_end()
        v = self._vi
        kernels, biases = self._unflatten(v["loc"].detach().clone())
        self._mlp.weights, self._mlp.biases = kernels, biases
        if v["rho"] is not None:
            self._post_rho = list(zip(*self._unflatten(v["rho"].detach().clone())))
        self._prior_loc = torch.zeros_like(v["loc"]).detach() if v["prior"] is None else v["prior"].detach()

    def kl_divergence(self) -> float:
        """Exact ``sum KL(q || p)`` of the current posterior over every weight against the prior
        ``Normal(prior means, prior_scale)``, summed in fp64 by the mean-field kernel."""
        loc, rho, prior = self._posterior_flat(ops._device())
        eps = None if rho is None else torch.zeros_like(loc)
        _, kl = ops.mean_field_draw_kl(loc, rho, eps, prior, self.prior_scale, kl_exact=True, want_w=False)
        return float(kl[0].item())

    def _last_layer_draws(self, x, n_draws: int):
        """Per posterior draw: the last hidden activations and the sampled output layer,
        ``h (S, B, H)``, ``W (S, H, P)``, ``b (S, P)`` (every layer re-sampled per draw,
        ``BayesianNNEstimator.py:122-145``)."""
        x = ops.as_device_f32(x)
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        if self._mlp is None:
            self._build(int(x.shape[-1]))
        dev = x.device
        self._mlp.to(dev)
        if self._draw_gen is None:
            self._draw_gen = torch.Generator(device=dev).manual_seed(self.random_seed)
        xm = torch.as_tensor(self.x_mean, dtype=torch.float32, device=dev)
        xs = torch.as_tensor(self.x_std, dtype=torch.float32, device=dev)
        xn = (x - xm) / (xs + 1e-8)
        act = _ACTIVATIONS[self.activation]
        scales = self.posterior_scales(dev)
        hs, ws, bs = [], [], []
        n = len(self._mlp.weights)
        for _ in range(n_draws):
            h = xn
            for i, (w, b) in enumerate(zip(self._mlp.weights, self._mlp.biases)):
                if scales is not None:  # a sample of q(w) = N(loc, scale^2), map mode: the mean
                    sw, sb = scales[i]
                    w = w + sw * torch.randn(w.shape, generator=self._draw_gen, device=dev, dtype=torch.float32)
                    b = b + sb * torch.randn(b.shape, generator=self._draw_gen, device=dev, dtype=torch.float32)
                if i < n - 1:
                    h = act(h @ w + b)
                else:
                    hs.append(h)
                    ws.append(w)
                    bs.append(b)
        return torch.stack(hs).contiguous(), torch.stack(ws).contiguous(), torch.stack(bs).contiguous()

    def evaluate(self, x, y, batch_size=None, verbose=0, include_kl=False, **kwargs) -> float:
        """Keras ``evaluate`` of ``BayesianNNEstimator``'s compiled loss for ONE posterior
        draw (every ``DenseVariational`` re-samples its weights per call,
        ``BayesianNNEstimator.py:122-145``): the mean NLL of (x, y) under ``t`` of a fresh
        draw.  With ``include_kl`` the layers' regularisation losses are added as Keras does:
        ``kl_weight_scale * KL(q || p)``, in the estimator's ``kl_use_exact`` form and, for the
        sampled form, at the very draw the NLL is evaluated at.  Both variants consume the draw
        generator identically."""
        x = np.asarray(x, np.float32) if not isinstance(x, torch.Tensor) else x
        y = np.asarray(y, np.float32) if not isinstance(y, torch.Tensor) else y
        if include_kl:
            dev = ops._device()
            if self._draw_gen is None:  # as _last_layer_draws creates it
                self._draw_gen = torch.Generator(device=dev).manual_seed(self.random_seed)
            before = self._draw_gen.get_state()
        with torch.no_grad():
            t = self.params_draws(x, 1)[0]
            nll = self._get_neg_log_likelihood()(y, self.dist_layer(t))
        value = float(nll.double().mean().item())
        if not include_kl:
            return value
        if self.kl_use_exact:
            return value + self.kl_weight_scale * self.kl_divergence()
        loc, rho, prior = self._posterior_flat(dev)
        eps = None
        if rho is not None:  # the draw's eps again: the layers' randn calls, replayed from the state before it
            after = self._draw_gen.get_state()
            self._draw_gen.set_state(before)
            eps = torch.cat([torch.randn(t_.shape, generator=self._draw_gen, device=dev).reshape(-1)
                             for pair in zip(self._mlp.weights, self._mlp.biases) for t_ in pair])
            self._draw_gen.set_state(after)
        _, kl = ops.mean_field_draw_kl(loc, rho, eps, prior, self.prior_scale, kl_exact=False, want_w=False)
        return value + self.kl_weight_scale * float(kl[0].item())

    def params_draws(self, x, n_draws: int) -> torch.Tensor:
        """``t`` for ``n_draws`` posterior weight samples: (S, B, P)."""
        h, W, b = self._last_layer_draws(x, n_draws)
        return torch.matmul(h, W) + b[:, None, :]

    def score(self, x_data, y_data, n_draws: Optional[int] = None) -> float:
        """``BayesianNNEstimator.py:65-76``: 50 draws (1 in map mode).  The S networks are
        drawn once; ``t`` of every draw is formed by the batched library GEMM and scored by the
        layer's fused posterior kernel, in row chunks that keep the (S, rows, P) tensor at or
        under ``POSTERIOR_CHUNK_BYTES``.  The chunks' {sum, non-finite count} pairs are added
        in fp64 on the device."""
        S = n_draws if n_draws is not None else (1 if self.map_mode else 50)
        y = ops.as_device_f32(np.asarray(y_data, np.float32))
        n = int(y.shape[0])
        with torch.no_grad():
            h, W, b = self._last_layer_draws(np.asarray(x_data, np.float32), S)
            rows = max(1, POSTERIOR_CHUNK_BYTES // (4 * S * int(W.shape[-1])))
            s = nf = None
            for r0 in range(0, n, rows):
                t = torch.matmul(h[:, r0:r0 + rows], W) + b[:, None, :]
                _, cs, cnf = self.dist_layer.posterior_lse(y[r0:r0 + rows], t, self.y_mean, self.y_std,
                                                           want_values=False, want_sum=True, want_nonfinite=True)
                s, nf = (cs, cnf) if s is None else (s + cs, nf + cnf)
        return self._finish_score(s, nf, n)


class BayesNormalizingFlowNetwork(BayesianNNEstimator):
    """``estimators/BayesNormalizingFlowNetwork.py`` over :class:`BayesianNNEstimator`.  ``score``
    stacks the S draws' last hidden activations and output-layer weights and evaluates
    ``logsumexp_s(log_pdf) - log S`` per sample in ONE fused kernel
    (``nfn_posterior_lse_dense_f32``, the output DenseVariational layer fused; or
    ``nfn_posterior_lse_f32`` over a library-GEMM ``t``) instead of S model re-runs."""

    def __init__(self, n_dims, kl_weight_scale=1.0, n_flows=2, trainable_base_dist=True, flow_types=None,
                 hidden_sizes=(10,), activation="tanh", noise_reg=("fixed_rate", 0.0), learning_rate=2e-2,
                 map_mode=False, prior_scale=1.0, trainable_prior=False, kl_use_exact=True, random_seed=22,
                 n_dims_x=None):
        flow_types = tuple(flow_types) if flow_types is not None else ("radial",) * n_flows
        dist_layer = InverseNormalizingFlowLayer(flow_types=flow_types, n_dims=n_dims,
                                                 trainable_base_dist=trainable_base_dist)
        super().__init__(dist_layer, kl_weight_scale, kl_use_exact=kl_use_exact, hidden_sizes=hidden_sizes,
                         activation=activation, learning_rate=learning_rate, noise_reg=noise_reg,
                         trainable_prior=trainable_prior, map_mode=map_mode, prior_scale=prior_scale,
                         random_seed=random_seed, n_dims_x=n_dims_x)

    def score(self, x_data, y_data, n_draws: Optional[int] = None) -> float:
        """``BayesianNNEstimator.py:65-76``: 50 draws (1 in map mode).  The output layer is
        fused into the posterior kernel (``nfn_posterior_lse_dense_f32``: t_s = h_s W_s + b_s
        never written to memory) when its width allows, else t is formed by the library GEMM."""
        S = n_draws if n_draws is not None else (1 if self.map_mode else 50)
        h, W, b = self._last_layer_draws(np.asarray(x_data, np.float32), S)
        _, s, nf = ops.posterior_lse_dense(np.asarray(y_data, np.float32), h, W, b, self.dist_layer.flow_types,
                                           self.n_dims, self.dist_layer.trainable_base_dist, self.y_mean,
                                           self.y_std, want_values=False, want_sum=True, want_nonfinite=True)
        return self._finish_score(s, nf, int(np.shape(y_data)[0]))


class BayesMixtureDensityNetwork(BayesianNNEstimator):
    """``estimators/BayesMixtureDensityNetwork.py``: the Bayesian net over a
    ``GaussianMixtureLayer``.  ``score`` is the fused posterior kernel
    ``nfn_posterior_lse_gaussian_mixture_f32``.  ``fit`` trains the posterior means by maximum
    likelihood through the fused mixture backward; ``fit(variational=True)`` trains the
    reference's variational objective (``BayesianNNEstimator.fit``)."""

    def __init__(self, n_dims, kl_weight_scale, n_centers=5, **kwargs):
        dist_layer = GaussianMixtureLayer(n_centers=n_centers, n_dims=n_dims)
        super().__init__(dist_layer, kl_weight_scale, **kwargs)

    @staticmethod
    def build_function(n_dims, kl_weight_scale, n_centers=5, kl_use_exact=True, hidden_sizes=(10,),
                       activation="tanh", noise_reg=("fixed_rate", 0.0), learning_rate=2e-2, trainable_prior=False,
                       map_mode=False, prior_scale=1.0):
        return BayesMixtureDensityNetwork(n_dims=n_dims, kl_weight_scale=kl_weight_scale, n_centers=n_centers,
                                          kl_use_exact=kl_use_exact, hidden_sizes=hidden_sizes,
                                          activation=activation, noise_reg=noise_reg, learning_rate=learning_rate,
                                          trainable_prior=trainable_prior, map_mode=map_mode,
                                          prior_scale=prior_scale)


class BayesKernelMixtureNetwork(BayesianNNEstimator):
    """``estimators/BayesKernelMixtureNetwork.py``: the Bayesian net over a
    ``GaussianKernelsLayer``.  ``score`` is the fused posterior kernel
    ``nfn_posterior_lse_kernel_mixture_f32``.  ``fit`` trains the posterior means (and the
    layer's bandwidth variable) by maximum likelihood through the fused mixture backward;
    ``fit(variational=True)`` trains the reference's variational objective
    (``BayesianNNEstimator.fit``)."""

    def __init__(self, n_dims, kl_weight_scale, n_centers=50, **kwargs):
        dist_layer = GaussianKernelsLayer(n_centers=n_centers, n_dims=n_dims, trainable_scale=True)
        super().__init__(dist_layer, kl_weight_scale, **kwargs)

    @staticmethod
    def build_function(n_dims, kl_weight_scale, n_centers=50, kl_use_exact=True, hidden_sizes=(10,),
                       activation="tanh", noise_reg=("fixed_rate", 0.0), learning_rate=2e-2, trainable_prior=False,
                       map_mode=False, prior_scale=1.0):
        return BayesKernelMixtureNetwork(n_dims=n_dims, kl_weight_scale=kl_weight_scale, n_centers=n_centers,
                                         kl_use_exact=kl_use_exact, hidden_sizes=hidden_sizes,
                                         activation=activation, noise_reg=noise_reg, learning_rate=learning_rate,
                                         trainable_prior=trainable_prior, map_mode=map_mode,
                                         prior_scale=prior_scale)

    def fit(self, x, y, batch_size=None, epochs=None, verbose=1, variational=False, **kwargs):
        """``BayesKernelMixtureNetwork.py:47-51``: the kernel centres are set from the normalised
        targets, then the posterior trains as in ``BayesianNNEstimator.fit``."""
        y = np.asarray(y, np.float32)
        y_mean = np.mean(y, axis=0, dtype=np.float32)
        y_std = np.std(y, axis=0, dtype=np.float32)
        self.dist_layer.set_center_points((y - y_mean) / y_std, seed=int(self.random_seed))
        return super().fit(x, y, batch_size=batch_size, epochs=epochs, verbose=verbose, variational=variational,
                           **kwargs)
