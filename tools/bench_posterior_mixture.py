"""Time the fused posterior score of a mixture layer (``nfn_posterior_lse_gaussian_mixture_f32``
/ ``nfn_posterior_lse_kernel_mixture_f32``) against the best composition the library offered
before it, on one GPU, in one run.

    python tools/bench_posterior_mixture.py --layer gmm --B 131072 --S 64 --K 5 --d 1
    python tools/bench_posterior_mixture.py --layer kernel --B 131072 --S 64 --M 100 --d 1

The composition: S calls of the fused single-draw op, each writing its row of an (S, B) tensor,
then ``torch.logsumexp(dim=0) - log S``.  Timing as tools/bench_mdn.py: warm-up launches, then
``--iters`` (>= 20) launches timed with device events around the whole window.  Fused and
composed windows alternate ``--repeats`` times and each number is the median.  Prints one JSON
line: ms per score, the fraction of the 8 TB/s HBM spec on the ALGORITHMIC bytes
``4 (S B width + B d + B)`` (plus ``4 M (d + 1)`` for the kernel layer's centres and
bandwidths), and the maximum difference between the two results."""

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from normalizingflownetwork_amd import ops  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8e12


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
    ap.add_argument("--layer", choices=("gmm", "kernel"), required=True)
    ap.add_argument("--B", type=int, default=1 << 17)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--K", type=int, default=5, help="components of the Gaussian mixture (--layer gmm)")
    ap.add_argument("--M", type=int, default=100, help="kernels of the kernel mixture (--layer kernel)")
    ap.add_argument("--d", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert args.iters >= 20, "time at least 20 launches"
    assert torch.cuda.is_available(), "bench_posterior_mixture needs a HIP device"
    dev = torch.device("cuda", 0)
    B, S, d = args.B, args.S, args.d
    g = torch.Generator(device=dev).manual_seed(22)
    y = torch.randn((B, d), generator=g, device=dev)
    if args.layer == "gmm":
        K = args.K
        width = K * (2 * d + 1)
        rows = torch.empty((S, B, width), device=dev)
        blocks = rows[:, :, :2 * K * d].view(S, B, K, 2, d)
        blocks[:, :, :, 0, :] = torch.rand((S, B, K, d), generator=g, device=dev) * 4.0 - 2.0
        blocks[:, :, :, 1, :] = 10.0 * torch.randn((S, B, K, d), generator=g, device=dev)
        rows[:, :, 2 * K * d:] = 3.0 * torch.randn((S, B, K), generator=g, device=dev)
        del blocks
        extra = 0

        def fused():
            return ops.posterior_lse_gaussian_mixture(y, rows, K, d)[0]

        def single(s):
            return ops.gaussian_mixture_log_prob(y, rows[s], K, d)[0]
    else:
        M = width = args.M
        rows = 3.0 * torch.randn((S, B, M), generator=g, device=dev)
        locs = torch.rand((M, d), generator=g, device=dev) * 4.0 - 2.0
        scales = torch.where(torch.arange(M, device=dev) < (M + 1) // 2, -0.3571, 0.3138).float()
        extra = 4 * M * (d + 1)

        def fused():
            return ops.posterior_lse_kernel_mixture(y, rows, locs, scales)[0]

        def single(s):
            return ops.kernel_mixture_log_prob(y, rows[s], locs, scales)[0]

    stack = torch.empty((S, B), device=dev)
    log_s = math.log(S)

    def composed():
        for s in range(S):
            stack[s] = single(s)
        return torch.logsumexp(stack, dim=0) - log_s

    check = (fused() - composed()).abs().max().item()
    fused_runs, composed_runs = [], []
    for _ in range(args.repeats):
        fused_runs.append(time_ms(fused, args.warmup, args.iters))
        composed_runs.append(time_ms(composed, args.warmup, args.iters))
    fused_ms, composed_ms = statistics.median(fused_runs), statistics.median(composed_runs)
    algo_bytes = 4 * (S * B * width + B * d + B) + extra
    print(json.dumps({
        "tool": "bench_posterior_mixture", "layer": args.layer, "B": B, "S": S, "width": width, "d": d,
        "iters": args.iters, "repeats": args.repeats, "fused_ms": round(fused_ms, 4),
        "composed_ms": round(composed_ms, 4), "fused_runs_ms": [round(v, 4) for v in fused_runs],
        "composed_runs_ms": [round(v, 4) for v in composed_runs],
        "speedup_vs_composed": round(composed_ms / fused_ms, 2), "algorithmic_bytes": algo_bytes,
        "fraction_of_8TBps": round(algo_bytes / (fused_ms * 1e-3) / HBM_SPEC_BYTES_PER_S, 4),
        "max_abs_diff_vs_composed": check, "fused_beats_composed": bool(fused_ms < composed_ms),
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
