"""Time the fused Gaussian-mixture log_prob of the mixture density network
(``nfn_gaussian_mixture_logprob_f32``) or its backward against the same expression composed
from torch ops, on one GPU, in one run.

    python tools/bench_mdn.py --B 4194304 --K 5 --d 1 --mode fwd|grad

Warm-up launches, then ``--iters`` (>= 20) launches timed with device events around the whole
window (one synchronise at the end).  Prints one JSON line: ms per launch, the fraction of the
8 TB/s HBM spec on the ALGORITHMIC bytes — with ``P = K (2 d + 1)``, forward ``4 B (P + d + 1)``
(t and y in, log_prob out), gradient that plus ``4 B (P + d)`` (grad_t and grad_y out) — and
the time of the torch composition.  The fused kernel must beat the composition, which moves
several times the bytes."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from normalizingflownetwork_amd import ops  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8e12
LOG_EXPM1_ONE = float(np.log(np.expm1(1.0)))


def torch_log_prob(y, t, K, d):
    blocks = t[:, :2 * K * d].reshape(-1, K, 2, d)
    loc, raw = blocks[:, :, 0, :], blocks[:, :, 1, :]
    logits = t[:, 2 * K * d:]
    sigma = torch.nn.functional.softplus(0.05 * raw + LOG_EXPM1_ONE)
    z = (y[:, None, :] - loc) / sigma
    c = -0.5 * (z * z).sum(-1) - torch.log(sigma).sum(-1) - 0.5 * d * float(np.log(2 * np.pi))
    return torch.logsumexp(logits + c, -1) - torch.logsumexp(logits, -1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1 << 22)
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--mode", choices=("fwd", "grad"), default="fwd")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert args.iters >= 20, "time at least 20 launches"
    assert torch.cuda.is_available(), "bench_mdn needs a HIP device"
    dev = torch.device("cuda", 0)
    B, K, d = args.B, args.K, args.d
    P = K * (2 * d + 1)
    g = torch.Generator(device=dev).manual_seed(22)
    y = torch.randn((B, d), generator=g, device=dev)
    t = torch.empty((B, P), device=dev)
    blocks = t[:, :2 * K * d].view(B, K, 2, d)
    blocks[:, :, 0, :] = torch.rand((B, K, d), generator=g, device=dev) * 4.0 - 2.0
    blocks[:, :, 1, :] = 10.0 * torch.randn((B, K, d), generator=g, device=dev)
    t[:, 2 * K * d:] = 3.0 * torch.randn((B, K), generator=g, device=dev)
    del blocks
    gout = torch.randn((B,), generator=g, device=dev)
    algo_bytes = 4 * B * (P + d + 1) + (4 * B * (P + d) if args.mode == "grad" else 0)

    if args.mode == "fwd":
        def fused():
            return ops.gaussian_mixture_log_prob(y, t, K, d)[0]

        def composed():
            with torch.no_grad():
                return torch_log_prob(y, t, K, d)

        check = (fused() - composed()).abs().max().item()
    else:
        def fused():
            return ops.gaussian_mixture_log_prob_grad(y, t, K, d, g_out=gout)

        def composed():
            yy, tt = (a.detach().requires_grad_(True) for a in (y, t))
            (torch_log_prob(yy, tt, K, d) * gout).sum().backward()
            return tt.grad, yy.grad

        check = (fused()[1] - composed()[0]).abs().max().item()
    fused_ms = time_ms(fused, args.warmup, args.iters)
    torch_ms = time_ms(composed, args.warmup, args.iters)
    print(json.dumps({
        "tool": "bench_mdn", "mode": args.mode, "B": B, "K": K, "d": d, "P": P, "iters": args.iters,
        "fused_ms": round(fused_ms, 4), "torch_ms": round(torch_ms, 4),
        "speedup_vs_torch": round(torch_ms / fused_ms, 2), "algorithmic_bytes": algo_bytes,
        "fraction_of_8TBps": round(algo_bytes / (fused_ms * 1e-3) / HBM_SPEC_BYTES_PER_S, 4),
        "max_abs_diff_vs_torch": check, "fused_beats_torch": bool(fused_ms < torch_ms),
    }), flush=True)
    return 0 if fused_ms < torch_ms else 1


if __name__ == "__main__":
    sys.exit(main())
