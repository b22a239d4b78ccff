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

``fit`` is an epoch loop around one ``_TrainStep`` (device data, generator, Adam, loss, the HIP
graph captured by ``ops.capture_graph``), which tests and ``tools/bench_variational.py`` build
too.  What it trains is the object ``_trainables`` hands it: ``_PointWeights`` (the Dense stack's
weights) or ``_MeanFieldWeights`` (the flat ``loc`` / ``rho`` / prior means of a variational fit).

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


def _f32(v):
    """``v`` as it is when a tensor, else a float32 numpy array."""
    return v if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)


class _MLP:
    """Dense stack x -> t (``MaximumLikelihoodNNEstimator.py:37-44``) over the given per-layer
    ``weights`` (in, out) and ``biases``."""

    def __init__(self, weights, biases, activation: str):
        assert activation in _ACTIVATIONS, f"unknown activation {activation!r}"
        self.weights, self.biases, self.activation = list(weights), list(biases), activation
        self._device = None

    @classmethod
    def glorot(cls, n_in: int, hidden_sizes: Sequence[int], n_out: int, activation: str, seed: int):
        """Glorot-uniform weights and zero biases like Keras' ``Dense`` defaults."""
        assert type(hidden_sizes) in (tuple, list)
        g = torch.Generator().manual_seed(seed)
        sizes = [n_in] + list(hidden_sizes) + [n_out]
        weights, biases = [], []
        for a, b in zip(sizes[:-1], sizes[1:]):
            lim = float(np.sqrt(6.0 / (a + b)))
            weights.append((torch.rand((a, b), generator=g, dtype=torch.float32) * 2 - 1) * lim)
            biases.append(torch.zeros((b,), dtype=torch.float32))
        return cls(weights, biases, activation)

    def to(self, device):
        if self._device != device:
            self.weights = [w.to(device) for w in self.weights]
            self.biases = [b.to(device) for b in self.biases]
            self._device = device
        return self

    def hidden(self, x: torch.Tensor) -> torch.Tensor:
        """Activations entering the linear output layer (the fused Dense path's input)."""
        act = _ACTIVATIONS[self.activation]
        h = x
        for w, b in zip(self.weights[:-1], self.biases[:-1]):
            h = act(h @ w + b)
        return h.contiguous()

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.hidden(x) @ self.weights[-1] + self.biases[-1]


class _PointWeights:
    """What a maximum-likelihood step trains: the weights of ``mlp`` (on the training device), as leaves."""

    draw_size = None  # the step has no weight draw and no penalty term

    def __init__(self, mlp: _MLP):
        self.mlp = mlp
        self.parameters = [p.detach().requires_grad_(True) for p in mlp.weights + mlp.biases]
        nw = len(mlp.weights)
        mlp.weights, mlp.biases = self.parameters[:nw], self.parameters[nw:]

    def network(self, eps):
        """``(network, penalty)`` of one step: the x -> t network and what its loss adds to the NLL."""
        return self.mlp, None

    def finish(self):
        """Leave the trained values in the estimator."""
        self.mlp.weights = [p.detach() for p in self.mlp.weights]
        self.mlp.biases = [p.detach() for p in self.mlp.biases]


class _TrainStep:
    """The training step of ``est`` on the data ``x``, ``y`` (float32 matrices), over the
    ``trained`` object's parameters plus the density layer's own: the device data, the
    normalisation, the generator, Adam, the loss and its fp64 epoch sums, and (``capture``) the
    HIP graph of the full-batch step with its static inputs.  Every N(0, 1) number comes from
    ``gen`` in one fixed order — per epoch the permutation, per step the x noise, the y noise
    and the weight draw, each only when in use, by ``randn`` eagerly and by ``normal_`` into the
    graph's static buffers under replay — so the replayed and the eager loop train identically."""

    def __init__(self, est, x, y, trained, dev):
        self.est, self.trained, self.dev = est, trained, dev
        dl, mlp = est.dist_layer, est._mlp
        # Keras Adam defaults; capturable: step counts and bias corrections live on the device, so the same
        # optimizer runs eagerly and in the graph.  The layer's own tensors: the kernel mixture's bandwidths
        self.opt = torch.optim.Adam(trained.parameters + dl.trainable_parameters(dev),
                                    lr=getattr(est, "learning_rate", 3e-3), betas=(0.9, 0.999), eps=1e-7,
                                    capturable=True)
        # the output Dense layer can be fused into the flow chain's kernels only
        self.fused_dense = (isinstance(dl, InverseNormalizingFlowLayer) and len(mlp.weights) > 1 and est.fused_dense
                            and ops.dense_fusable(int(mlp.weights[-1].shape[0]), dl.get_total_param_size(), est.n_dims))
        self.X, self.Y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        self.xm, self.xs, self.ym, self.ys = (torch.as_tensor(v, dtype=torch.float32, device=dev)
                                              for v in (est.x_mean, est.x_std, est.y_mean, est.y_std))
        self.sum_log_ys = torch.log(self.ys).sum()
        self.gen = torch.Generator(device=dev).manual_seed(int(est.random_seed))
        self.acc = torch.zeros((), dtype=torch.float64, device=dev)
        self.acc_pen = torch.zeros((), dtype=torch.float64, device=dev) if trained.draw_size is not None else None
        self.graph = None  # ops.CapturedGraph of the full-batch step; idx, noise: its static inputs

    def begin_epoch(self, shuffle: bool) -> torch.Tensor:
        """The epoch's row order; the epoch sums start again."""
        n = self.X.shape[0]
        perm = torch.randperm(n, generator=self.gen, device=self.dev) if shuffle else torch.arange(n, device=self.dev)
        self.acc.zero_()
        if self.acc_pen is not None:
            self.acc_pen.zero_()
        return perm

    def draws(self, rows: int):
        """The step's normal draws ``(x noise, y noise, eps)``, in the order the replay refills them."""
        est, n_eps, gen, dev = self.est, self.trained.draw_size, self.gen, self.dev
        nx = torch.randn((rows, self.X.shape[1]), generator=gen, device=dev) if est.x_noise_std > 0 else None
        ny = torch.randn((rows, self.Y.shape[1]), generator=gen, device=dev) if est.y_noise_std > 0 else None
        eps = torch.randn((n_eps,), generator=gen, device=dev) if n_eps else None
        return nx, ny, eps

    def loss(self, idx, nx, ny, eps) -> torch.Tensor:
        """The loss on the rows ``idx`` with the noise draws ``nx`` / ``ny`` and the weight draw
        ``eps``; its penalty term is added to the epoch's penalty sum."""
        est, dl = self.est, self.est.dist_layer
        xn = (self.X[idx] - self.xm) / (self.xs + 1e-8)
        if nx is not None:
            xn = xn + est.x_noise_std * nx
        yc = (self.Y[idx] - self.ym) / self.ys
        if ny is not None:
            yc = yc + est.y_noise_std * ny
        mlp, penalty = self.trained.network(eps)
        if self.fused_dense:  # output layer fused into the chain, forward and backward
            lp = ops.log_prob_dense(yc, mlp.hidden(xn), mlp.weights[-1], mlp.biases[-1],
                                    dl.flow_types, est.n_dims, dl.trainable_base_dist)
        else:
            lp = dl.train_log_prob(yc, mlp(xn))  # the layer's differentiable fused log_prob
        loss = -lp.mean() + self.sum_log_ys
        if penalty is not None:
            loss = loss + penalty
            self.acc_pen.add_(penalty.detach().double() * idx.numel())
        return loss

    def run(self, idx, nx, ny, eps):
        """One training step: ``loss``, its gradients (the caller has cleared them) and Adam."""
        loss = self.loss(idx, nx, ny, eps)
        loss.backward()
        self.opt.step()
        self.acc.add_(loss.detach().double() * idx.numel())

    def capture(self, idx, noise, stream=None):
        """Capture the step on the batch ``idx`` with its ``draws`` ``noise``, which become the
        graph's static inputs.  The capture itself executes nothing: this batch then runs as
        the graph's first replay."""
        self.idx, self.noise = idx.clone(), noise
        self.opt.zero_grad(set_to_none=True)
        self.graph = ops.capture_graph(lambda: self.run(self.idx, *noise), self.dev, stream)
        self.graph.replay()

    def replay(self, idx):
        """The captured step on the rows ``idx`` with fresh draws."""
        self.idx.copy_(idx)
        for buf in self.noise:
            if buf is not None:
                buf.normal_(generator=self.gen)
        self.graph.replay()

    def epoch_sums(self):
        """``(loss, penalty | None)`` summed over the rows stepped since ``begin_epoch``."""
        return float(self.acc.item()), None if self.acc_pen is None else float(self.acc_pen.item())


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
        self._mlp = _MLP.glorot(n_dims_x, self.hidden_sizes, self.dist_layer.get_total_param_size(),
                                self.activation, self.random_seed)
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

    def _normalised_x(self, x, device=None) -> torch.Tensor:
        """``(x - mu_x)/(sigma_x + 1e-8)`` as a (B, n_dims_x) device tensor, with the MLP (built
        on first use) on the same device."""
        x = ops.as_device_f32(x, device)
        if x.dim() == 1:
            x = x.unsqueeze(-1)
        if self._mlp is None:
            self._build(int(x.shape[-1]))
        dev = x.device
        self._mlp.to(dev)
        xm = torch.as_tensor(self.x_mean, dtype=torch.float32, device=dev)
        xs = torch.as_tensor(self.x_std, dtype=torch.float32, device=dev)
        return (x - xm) / (xs + 1e-8)

    def params(self, x) -> torch.Tensor:
        """``t = MLP((x - mu_x)/(sigma_x + 1e-8))`` (``MaximumLikelihoodNNEstimator.py:40-43``)."""
        xn = self._normalised_x(x)  # first: it may build the MLP
        return self._mlp(xn).contiguous()

    def __call__(self, x):
        return self.dist_layer(self.params(x))

    def _fused_dense_inputs(self, x):
        """``(h, W, b)`` of the output Dense layer when the fused Dense->chain kernel takes
        the shapes (evaluation only: no autograd through it), else None."""
        if not isinstance(self.dist_layer, InverseNormalizingFlowLayer):
            return None  # the fused Dense kernels evaluate a flow chain
        if torch.is_grad_enabled() and any(w.requires_grad for w in (self._mlp.weights if self._mlp else [])):
            return None
        xn = self._normalised_x(x)
        W, b = self._mlp.weights[-1], self._mlp.biases[-1]
        if not ops.dense_fusable(int(W.shape[0]), int(W.shape[1]), self.n_dims) or len(self._mlp.weights) < 2:
            return None
        return self._mlp.hidden(xn), W, b

    def call(self, x, training=False):
        return self(x)

    # --- evaluation ---------------------------------------------------------------
    def log_pdf(self, x, y):
        """``BaseEstimator.py:77-86``: ``log_prob((y-mu)/sigma) - sum(log sigma)``."""
        x, y = _f32(x), _f32(y)
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
        x_data, y_data = _f32(x_data), _f32(y_data)
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
        x, y = _f32(x), _f32(y)
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
        step = self._train_step(x, y, **kwargs)
        n = step.X.shape[0]
        batch_size = 32 if batch_size is None else int(batch_size)
        epochs = 1 if epochs is None else int(epochs)
        warm = 3  # eager steps before the capture (optimizer state, allocator pools)
        steps_done = 0
        history = {"loss": []} if step.acc_pen is None else {"loss": [], "nll": [], "kl": []}
        try:
            for _ in range(epochs):
                perm = step.begin_epoch(shuffle)
                for i in range(0, n, batch_size):
                    idx = perm[i:i + batch_size]
                    full = idx.numel() == batch_size
                    if use_graph and full and step.graph is not None:
                        step.replay(idx)
                        continue
                    noise = step.draws(idx.numel())
                    if use_graph and full and steps_done >= warm:
                        step.capture(idx, noise)
                        continue
                    step.opt.zero_grad(set_to_none=True)
                    if use_graph and steps_done < warm:
                        with ops.side_stream(step.dev):  # warm-up on a side stream (capture rules)
                            step.run(idx, *noise)
                    else:
                        step.run(idx, *noise)
                    steps_done += 1
                loss_sum, pen_sum = step.epoch_sums()
                ep_loss = loss_sum / n
                history["loss"].append(ep_loss)
                if pen_sum is not None:  # loss = nll + kl, the weighted KL term as Keras adds it
                    ep_kl = pen_sum / n
                    history["kl"].append(ep_kl)
                    history["nll"].append(ep_loss - ep_kl)
                if verbose:
                    print(f"epoch {len(history['loss'])}/{epochs} loss {ep_loss:.6f}", flush=True)
                if not np.isfinite(ep_loss):  # tf.keras.callbacks.TerminateOnNaN
                    break
        finally:
            step.trained.finish()
            self.dist_layer.finish_training()
        return history

    def _train_step(self, x, y, **kwargs) -> _TrainStep:
        """The step ``fit`` runs on ``x``, ``y``: normalisation and noise scales assigned from the
        data, the network on the device, and what ``_trainables(dev, **kwargs)`` says to train."""
        x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
        assert len(x.shape) == len(y.shape) == 2, "Please pass a matrix not a vector"
        self._assign_data_normalization(x, y)
        self._assign_noise_regularisation(n_dims=x.shape[1] + y.shape[1], n_datapoints=x.shape[0])
        if self._mlp is None:
            self._build(int(x.shape[1]))
        dev = ops._device()
        self._mlp.to(dev)
        return _TrainStep(self, x, y, self._trainables(dev, **kwargs), dev)

    def _trainables(self, dev, **kwargs):
        """What a step trains (``parameters``, ``draw_size``, ``network(eps)``, ``finish()``): here
        the network's own weights; the Bayesian estimator's variational fit overrides it."""
        return _PointWeights(self._mlp)


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


class _CentresFromTargets:
    """``KernelMixtureNetwork.py:35-39`` / ``BayesKernelMixtureNetwork.py:47-51``: before the
    training step is set up, the kernel centres are set from the normalised targets."""

    def _train_step(self, x, y, **kwargs):
        y = np.asarray(y, np.float32)
        y_circ = (y - np.mean(y, axis=0, dtype=np.float32)) / np.std(y, axis=0, dtype=np.float32)
        self.dist_layer.set_center_points(y_circ, seed=int(self.random_seed))
        return super()._train_step(x, y, **kwargs)


class KernelMixtureNetwork(_CentresFromTargets, BaseEstimator):
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


class _MeanFieldWeights:
    """What a step of ``BayesianNNEstimator.fit(variational=True)`` trains: the reference's
    compiled model (``BayesianNNEstimator.py:42-63, 109-146``) on flat vectors.  Per step ONE
    ``eps ~ N(0, 1)`` for all weights (after the noise draws, from the same generator), the draw
    ``w = loc + s * eps`` and KL(q || p) in one fused launch (``draw_kl``; backward: one more),
    the layers' ``W``, ``b`` as views of ``w``, and ``loss = mean NLL + kl_weight_scale * KL`` —
    Keras adds each layer's ``kl_weight * KL`` to the batch-mean loss, and summing the layers
    first is the same number.  ``kl_use_exact``, ``prior_scale``, ``trainable_prior`` and
    ``map_mode`` act as in the reference.  One Adam covers ``loc``, ``rho`` (not in map mode),
    the prior means (``trainable_prior``) and the density layer's own tensors; the step replays
    from the same HIP graph, ``eps`` refilled in place.  ``history`` then also holds ``"nll"``
    and ``"kl"`` (the weighted term), ``"loss"`` being their sum."""

    def __init__(self, est, dev, draw_kl=ops.mean_field_draw_kl_diff):
        self.est, self.draw_kl = est, draw_kl
        self.loc, self.rho, self.prior = est._posterior_flat(dev)
        if self.prior is None and est.trainable_prior:
            self.prior = torch.zeros_like(self.loc)
        self.parameters = ([self.loc] + ([] if self.rho is None else [self.rho])
                           + ([self.prior] if est.trainable_prior else []))
        for p in self.parameters:
            p.requires_grad_(True)
        # length of the N(0, 1) draw a step takes after its noise draws (0, map mode: a penalty, no draw)
        self.draw_size = 0 if self.rho is None else int(self.loc.numel())

    def network(self, eps):
        """This step's network, the drawn weights in the Dense stack's shapes, and the weighted KL."""
        est = self.est
        w, kl = self.draw_kl(self.loc, self.rho, eps, self.prior, est.prior_scale, est.kl_use_exact)
        return _MLP(*est._unflatten(w), est.activation), est.kl_weight_scale * kl

    def finish(self):
        """Write the flat vectors back into the estimator's per-layer layout."""
        est = self.est
        est._mlp.weights, est._mlp.biases = est._unflatten(self.loc.detach().clone())
        if self.rho is not None:
            est._post_rho = list(zip(*est._unflatten(self.rho.detach().clone())))
        est._prior_loc = torch.zeros_like(self.loc).detach() if self.prior is None else self.prior.detach()


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

    def _trainables(self, dev, variational=False, **kwargs):
        """``fit(variational=True)`` trains the mean-field posterior (:class:`_MeanFieldWeights`);
        by default the posterior means train by maximum likelihood."""
        return _MeanFieldWeights(self, dev) if variational else super()._trainables(dev)

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
        xn = self._normalised_x(x)
        dev = xn.device
        gen = self._draw_generator(dev)
        scales = self.posterior_scales(dev)
        hs, ws, bs = [], [], []
        for _ in range(n_draws):
            net = self._mlp
            if scales is not None:  # a sample of q(w) = N(loc, scale^2) per layer; map mode: the mean
                drawn = [(w + sw * torch.randn(w.shape, generator=gen, device=dev, dtype=torch.float32),
                          b + sb * torch.randn(b.shape, generator=gen, device=dev, dtype=torch.float32))
                         for w, b, (sw, sb) in zip(net.weights, net.biases, scales)]
                net = _MLP(*zip(*drawn), self.activation)
            hs.append(net.hidden(xn))
            ws.append(net.weights[-1])
            bs.append(net.biases[-1])
        return torch.stack(hs).contiguous(), torch.stack(ws).contiguous(), torch.stack(bs).contiguous()

    def _draw_generator(self, dev) -> torch.Generator:
        """The generator of the posterior draws (``_draw_gen``), seeded on first use."""
        if self._draw_gen is None:
            self._draw_gen = torch.Generator(device=dev).manual_seed(self.random_seed)
        return self._draw_gen

    def evaluate(self, x, y, batch_size=None, verbose=0, include_kl=False, **kwargs) -> float:
        """Keras ``evaluate`` of ``BayesianNNEstimator``'s compiled loss for ONE posterior
        draw (every ``DenseVariational`` re-samples its weights per call,
        ``BayesianNNEstimator.py:122-145``): the mean NLL of (x, y) under ``t`` of a fresh
        draw.  With ``include_kl`` the layers' regularisation losses are added as Keras does:
        ``kl_weight_scale * KL(q || p)``, in the estimator's ``kl_use_exact`` form and, for the
        sampled form, at the very draw the NLL is evaluated at.  Both variants consume the draw
        generator identically."""
        x, y = _f32(x), _f32(y)
        if include_kl:
            dev = ops._device()
            before = self._draw_generator(dev).get_state()
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

    def _n_draws(self, n_draws: Optional[int]) -> int:
        """``BayesianNNEstimator.py:65-76``: 50 posterior draws by default, 1 in map mode."""
        return n_draws if n_draws is not None else (1 if self.map_mode else 50)

    def score(self, x_data, y_data, n_draws: Optional[int] = None) -> float:
        """``BayesianNNEstimator.py:65-76``: 50 draws (1 in map mode).  The S networks are
        drawn once; ``t`` of every draw is formed by the batched library GEMM and scored by the
        layer's fused posterior kernel, in row chunks that keep the (S, rows, P) tensor at or
        under ``POSTERIOR_CHUNK_BYTES``.  The chunks' {sum, non-finite count} pairs are added
        in fp64 on the device."""
        S = self._n_draws(n_draws)
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
        h, W, b = self._last_layer_draws(np.asarray(x_data, np.float32), self._n_draws(n_draws))
        _, s, nf = ops.posterior_lse_dense(np.asarray(y_data, np.float32), h, W, b, self.dist_layer.flow_types,
                                           self.n_dims, self.dist_layer.trainable_base_dist, self.y_mean,
                                           self.y_std, want_values=False, want_sum=True, want_nonfinite=True)
        return self._finish_score(s, nf, int(np.shape(y_data)[0]))


class BayesMixtureDensityNetwork(BayesianNNEstimator):
    """``estimators/BayesMixtureDensityNetwork.py``: the Bayesian net over a
    ``GaussianMixtureLayer``.  ``score`` is the fused posterior kernel
    ``nfn_posterior_lse_gaussian_mixture_f32``.  ``fit`` trains the posterior means by maximum
    likelihood through the fused mixture backward; ``fit(variational=True)`` trains the
    reference's variational objective (``_MeanFieldWeights``)."""

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


class BayesKernelMixtureNetwork(_CentresFromTargets, BayesianNNEstimator):
    """``estimators/BayesKernelMixtureNetwork.py``: the Bayesian net over a
    ``GaussianKernelsLayer``.  ``score`` is the fused posterior kernel
    ``nfn_posterior_lse_kernel_mixture_f32``.  ``fit`` sets the kernel centres, then trains the
    posterior means (and the layer's bandwidth variable) by maximum likelihood through the fused
    mixture backward; ``fit(variational=True)`` trains the reference's variational objective
    (``_MeanFieldWeights``)."""

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
