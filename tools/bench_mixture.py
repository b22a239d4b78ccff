"""Time the fused Gaussian-kernel mixture log_prob (``nfn_kernel_mixture_logprob_f32``) or its
backward against the same expression composed from torch ops, on one GPU, in one run.

    python tools/bench_mixture.py --B 4194304 --M 100 --d 1 --mode fwd|grad

Warm-up launches, then ``--iters`` (>= 20) launches timed with device events around the whole
window (one synchronise at the end).  Prints one JSON line: ms per launch, the fraction of the
8 TB/s HBM spec on the ALGORITHMIC bytes — forward ``4 B (M + d + 1)`` (logits and y in,
log_prob out), gradient that plus ``4 B (M + d)`` (grad_logits and grad_y out) — and the time
of the torch composition.  The fused kernel must beat the composition, which moves several
times the bytes."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from normalizingflownetwork_amd import ops  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8e12


def torch_log_prob(y, t, locs, s):
    d = locs.shape[1]
    z2 = (((y[:, None, :] - locs[None]) / s[None, :, None]) ** 2).sum(-1)
    c = -0.5 * z2 - d * torch.log(s.abs())[None, :] - 0.5 * d * float(np.log(2 * np.pi))
    return torch.logsumexp(t + c, -1) - torch.logsumexp(t, -1)


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
    ap.add_argument("--M", type=int, default=100)
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--mode", choices=("fwd", "grad"), default="fwd")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    assert args.iters >= 20, "time at least 20 launches"
    assert torch.cuda.is_available(), "bench_mixture needs a HIP device"
    dev = torch.device("cuda", 0)
    B, M, d = args.B, args.M, args.d
    g = torch.Generator(device=dev).manual_seed(22)
    y = torch.randn((B, d), generator=g, device=dev)
    t = 3.0 * torch.randn((B, M), generator=g, device=dev)
    locs = torch.rand((M, d), generator=g, device=dev) * 4.0 - 2.0
    half = (M + 1) // 2
    s = torch.cat([torch.full((half,), -0.3571, device=dev), torch.full((M - half,), 0.7068, device=dev)])
    gout = torch.randn((B,), generator=g, device=dev)
    algo_bytes = 4 * B * (M + d + 1) + (4 * B * (M + d) if args.mode == "grad" else 0)

    if args.mode == "fwd":
        def fused():
            return ops.kernel_mixture_log_prob(y, t, locs, s)[0]

        def composed():
            with torch.no_grad():
                return torch_log_prob(y, t, locs, s)

        check = (fused() - composed()).abs().max().item()
    else:
        def fused():
            return ops.kernel_mixture_log_prob_grad(y, t, locs, s, g_out=gout)

        def composed():
            yy, tt, ss = (a.detach().requires_grad_(True) for a in (y, t, s))
            (torch_log_prob(yy, tt, locs, ss) * gout).sum().backward()
            return tt.grad, yy.grad, ss.grad

        check = (fused()[1] - composed()[0]).abs().max().item()
    fused_ms = time_ms(fused, args.warmup, args.iters)
    torch_ms = time_ms(composed, args.warmup, args.iters)
    print(json.dumps({
        "tool": "bench_mixture", "mode": args.mode, "B": B, "M": M, "d": d, "iters": args.iters,
        "fused_ms": round(fused_ms, 4), "torch_ms": round(torch_ms, 4),
        "speedup_vs_torch": round(torch_ms / fused_ms, 2), "algorithmic_bytes": algo_bytes,
        "fraction_of_8TBps": round(algo_bytes / (fused_ms * 1e-3) / HBM_SPEC_BYTES_PER_S, 4),
        "max_abs_diff_vs_torch": check, "fused_beats_torch": bool(fused_ms < torch_ms),
    }), flush=True)
    return 0 if fused_ms < torch_ms else 1


if __name__ == "__main__":
    sys.exit(main())
