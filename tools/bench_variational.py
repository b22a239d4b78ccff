"""Time the fused mean-field kernels (``nfn_mean_field_draw_kl_f32`` and its backward) on one
GPU, in one run:

    python tools/bench_variational.py [--N 4194304] [--rounds 7] [--steps 1000]

(a) The kernels alone on a flat vector of ``--N`` weights with a prior mean: ms per launch over
    ``--iters`` (>= 20) launches timed with device events around the whole window, and the
    fraction of the 8 TB/s HBM spec on the ALGORITHMIC bytes — forward 16 B per element (loc, rho,
    eps in, w out) + 4 with a prior mean, backward 24 B per element (loc, rho, eps, g_w in, two
    gradients out) + 4 with a prior mean (grad_prior_loc is not written) — next to the same
    expressions composed from torch ops.
(b) The replayed variational training step of ``BayesNormalizingFlowNetwork(1, n_flows=2,
    hidden_sizes=(10,))`` at batch 32, the estimator's own ``_TrainStep`` as ``fit(variational=True)``
    captures it (gather, normalisation, draw + KL, MLP, fused log_prob forward and backward, Adam,
    the epoch sums), against the same step whose draw and KL are the torch-op formulation on the
    same flat vectors.  Both graphs live in this process and are timed alternately, ``--rounds``
    windows of ``--steps`` replays each (the index copy and ``eps`` refill included, as in ``fit``);
    the medians are reported.

Prints one JSON line per part."""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from normalizingflownetwork_amd import BayesNormalizingFlowNetwork, ops  # noqa: E402
from normalizingflownetwork_amd.estimators import _MeanFieldWeights, _TrainStep  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8e12
LOG_EXPM1_ONE = float(np.log(np.expm1(1.0)))


def torch_draw_kl(loc, rho, eps, prior_loc=None, prior_scale=1.0, kl_exact=True):
    """The draw and the exact KL composed from torch ops on the flat vectors."""
    assert kl_exact
    s = 1e-3 + torch.nn.functional.softplus(LOG_EXPM1_ONE + 0.05 * rho)
    w = loc + s * eps
    dm = loc if prior_loc is None else loc - prior_loc
    kl = (np.log(prior_scale) - torch.log(s) + (s * s + dm * dm) * (0.5 / prior_scale ** 2) - 0.5).sum()
    return w, kl


def time_ms(fn, warmup: int, iters: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def bench_kernels(N: int, warmup: int, iters: int, dev):
    g = torch.Generator(device=dev).manual_seed(22)
    loc, eps, prior, g_w = (torch.randn((N,), generator=g, device=dev) for _ in range(4))
    rho = 20.0 * torch.randn((N,), generator=g, device=dev)
    g_kl = torch.full((1,), 1.0 / 256, device=dev)

    def fused_fwd():
        return ops.mean_field_draw_kl(loc, rho, eps, prior)

    def fused_bwd():
        return ops.mean_field_draw_kl_grad(loc, rho, eps, prior, g_w=g_w, g_kl=g_kl)

    def torch_fwd():
        with torch.no_grad():
            return torch_draw_kl(loc, rho, eps, prior)

    def torch_bwd():
        m, r = (a.detach().requires_grad_(True) for a in (loc, rho))
        w, kl = torch_draw_kl(m, r, eps, prior)
        ((w * g_w).sum() + g_kl[0] * kl).backward()
        return m.grad, r.grad

    (w, kl), (tw, tkl) = fused_fwd(), torch_fwd()
    check_w = (w - tw).abs().max().item()
    check_kl = abs(kl[0].item() - tkl.item()) / abs(kl[0].item())
    check_g = max((a - b).abs().max().item() for a, b in zip(fused_bwd()[:2], torch_bwd()))
    out = {"tool": "bench_variational", "part": "kernels", "N": N, "iters": iters,
           "max_abs_diff_w_vs_torch": check_w, "rel_diff_kl_vs_torch": check_kl, "max_abs_diff_grad_vs_torch": check_g}
    for name, fused, composed, bytes_per in (("fwd", fused_fwd, torch_fwd, 20), ("bwd", fused_bwd, torch_bwd, 28)):
        f_ms, t_ms = time_ms(fused, warmup, iters), time_ms(composed, warmup, iters)
        out.update({f"{name}_fused_ms": round(f_ms, 4), f"{name}_torch_ms": round(t_ms, 4),
                    f"{name}_algorithmic_bytes": bytes_per * N,
                    f"{name}_fraction_of_8TBps": round(bytes_per * N / (f_ms * 1e-3) / HBM_SPEC_BYTES_PER_S, 4)})
    print(json.dumps(out), flush=True)


class ReplayedStep:
    """One model's variational training step as ``fit(variational=True)`` runs and captures it
    (the estimator's ``_TrainStep``); ``draw_kl`` is the differentiable draw + KL the step uses."""

    def __init__(self, draw_kl, x, y, batch: int, dev):
        m = BayesNormalizingFlowNetwork(1, kl_weight_scale=1.0 / x.shape[0], n_flows=2, hidden_sizes=(10,))
        m._assign_data_normalization(x, y)
        m._build(1)
        m._mlp.to(dev)
        self.batch = batch
        self.step = step = _TrainStep(m, x, y, _MeanFieldWeights(m, dev, draw_kl), dev)
        self.idx = step.begin_epoch(shuffle=True)[:batch]
        with ops.side_stream(dev) as side:  # fit's three eager steps before the capture
            for _ in range(3):
                step.opt.zero_grad(set_to_none=True)
                step.run(self.idx, *step.draws(batch))
        step.capture(self.idx, step.draws(batch), stream=side)

    def replay(self):
        self.step.replay(self.idx)

    def last_loss(self) -> float:
        """The loss of one more replayed step, from the step's fp64 sum."""
        before = self.step.epoch_sums()[0]
        self.replay()
        return (self.step.epoch_sums()[0] - before) / self.batch


def bench_step(rounds: int, steps: int, batch: int, dev):
    rng = np.random.default_rng(22)
    x = rng.uniform(-3, 3, (256, 1)).astype(np.float32)
    y = (np.cos(x) + 0.3 * rng.standard_normal((256, 1))).astype(np.float32)
    variants = {"fused": ReplayedStep(ops.mean_field_draw_kl_diff, x, y, batch, dev),
                "torch": ReplayedStep(torch_draw_kl, x, y, batch, dev)}
    times = {k: [] for k in variants}
    for v in variants.values():
        for _ in range(50):
            v.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, v in variants.items():  # alternating windows in one process
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(steps):
                v.replay()
            stop.record()
            torch.cuda.synchronize()
            times[name].append(start.elapsed_time(stop) / steps * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "tool": "bench_variational", "part": "replayed_step", "model": "BayesNormalizingFlowNetwork(1, n_flows=2, "
        "hidden_sizes=(10,))", "batch": batch, "weights": variants["fused"].step.trained.draw_size, "rounds": rounds,
        "steps_per_round": steps, "fused_us_per_step": round(med["fused"], 2),
        "torch_us_per_step": round(med["torch"], 2),
        "fused_us_min_max": [round(min(times["fused"]), 2), round(max(times["fused"]), 2)],
        "torch_us_min_max": [round(min(times["torch"]), 2), round(max(times["torch"]), 2)],
        "speedup_vs_torch": round(med["torch"] / med["fused"], 3),
        "final_loss": {k: v.last_loss() for k, v in variants.items()},
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    assert args.iters >= 20, "time at least 20 launches"
    assert torch.cuda.is_available(), "bench_variational needs a HIP device"
    dev = torch.device("cuda", 0)
    bench_kernels(args.N, args.warmup, args.iters, dev)
    bench_step(args.rounds, args.steps, args.batch, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
