"""Output Dense layer fused into the chain: t = h W + b on
chip (fp32 MFMA), then the chain — against the oracle on t computed in fp64 / fp32."""

import os

import numpy as np
import pytest
import torch

from oracle import nfn_oracle as O
from parity import check_bound, check_forward, check_grad, fp32_sensitivity

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["fast", "precise"])
def math_mode(request, gpu):
    from normalizingflownetwork_amd import ops

    prev = ops.set_math_mode(request.param)
    yield request.param
    ops.set_math_mode(prev)


def _case(ft, d, H, B, seed, bias=True):
    rng = np.random.default_rng(seed)
    P = O.total_param_size(ft, d, True)
    h = rng.standard_normal((B, H)).astype(np.float32)
    W = (rng.standard_normal((H, P)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(P)).astype(np.float32) if bias else None
    y = rng.standard_normal((B, d)).astype(np.float32)
    t64 = h.astype(np.float64) @ W.astype(np.float64) + (0 if b is None else b.astype(np.float64))
    t32 = (h @ W + (0 if b is None else b)).astype(np.float32)
    return h, W, b, y, t64, t32


@pytest.mark.parametrize("ft,d,H,B", [(("planar", "radial") * 5, 1, 16, 1000), (("radial", "radial"), 1, 4, 333),
                                      (("planar", "radial") * 5, 1, 64, 777), (("affine", "planar", "radial"), 3, 8, 300),
                                      (("radial",) * 10, 1, 32, 64), (("planar", "affine"), 8, 16, 129),
                                      # d = 1 with 3 and 4 sixteen-column N tiles (P = 44, 50), H = 8 / 32
                                      (("radial",) * 14, 1, 8, 1001), (("planar", "radial") * 8, 1, 32, 700),
                                      # alternating / homogeneous programs of odd length (the compile-time
                                      # pair bodies, hpair_types): (P, R) x 3 + P, (R, P) x 4 + R, P x 5
                                      (("planar", "radial") * 3 + ("planar",), 1, 16, 500),
                                      (("radial", "planar") * 4 + ("radial",), 1, 8, 300),
                                      (("planar",) * 5, 1, 4, 257),
                                      # H = 16 with one sixteen-column N tile (P = 14): the split-bf16 t GEMM
                                      (("radial", "planar") * 2, 1, 16, 300)])
def test_dense_matches_oracle(math_mode, ft, d, H, B):
    from normalizingflownetwork_amd import ops

    h, W, b, y, t64, t32 = _case(ft, d, H, B, seed=H + B)
    out, s = ops.chain_log_prob_dense(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(), torch.from_numpy(W).cuda(),
                                      torch.from_numpy(b).cuda(), ft, d, True, want_sum=True)
    ref64 = O.chain_log_prob(y, t64, ft, d, True, np.float64)
    ref32 = O.chain_log_prob(y, t32, ft, d, True, np.float32)
    got = out.cpu().numpy()
    check_forward(got, ref64, ref32, f"dense {ft[:2]}x{len(ft)} d={d} H={H} B={B} [{math_mode}]", kind="dense",
                  sensitivity=fp32_sensitivity(y, t32, ft, d, True))
    bound = O.tolerance_bound(ref64, ref32)
    assert abs(s.item() - ref64.sum()) <= bound.sum() + 1e-6 * abs(ref64.sum())


@pytest.mark.parametrize("B,bias,hs", [(37, False, 16), (64 * 9 + 1, True, 20), (4096, False, 24)])
def test_dense_split_t_views_and_tails(gpu, B, bias, hs):
    """The split-bf16 t GEMM (H = 16, P <= 32: chain_dense1_kernel SB) on h row views of a wider
    buffer, with and without bias, on batches that end inside a tile (and one shorter than a
    tile), against the oracle on t = h W + b."""
    from normalizingflownetwork_amd import ops

    ft, d, H = ("planar", "radial") * 5, 1, 16
    h, W, b, y, t64, t32 = _case(ft, d, H, B, seed=B + hs, bias=bias)
    hbuf = np.zeros((B, hs), np.float32)
    hbuf[:, :H] = h
    hv = torch.from_numpy(hbuf).cuda()[:, :H]
    bb = None if b is None else torch.from_numpy(b).cuda()
    out, s = ops.chain_log_prob_dense(torch.from_numpy(y).cuda(), hv, torch.from_numpy(W).cuda(), bb, ft, d, True,
                                      want_sum=True)
    ref64 = O.chain_log_prob(y, t64, ft, d, True, np.float64)
    ref32 = O.chain_log_prob(y, t32, ft, d, True, np.float32)
    check_forward(out.cpu().numpy(), ref64, ref32, f"dense split-t views B={B} row stride {hs} bias={bias}",
                  kind="dense", sensitivity=fp32_sensitivity(y, t32, ft, d, True))
    bound = O.tolerance_bound(ref64, ref32)
    assert abs(s.item() - ref64.sum()) <= bound.sum() + 1e-6 * abs(ref64.sum())


def test_dense_with_normalisation_and_fallback(gpu):
    """With and without bias, with the fused y normalisation, and through the
    unsupported-shape fallback (H = 10: library GEMM + chain kernel), against the
    oracle's log_pdf on t = h W + b."""
    from normalizingflownetwork_amd import ops

    ft, d = ("planar", "radial") * 3, 1
    ym, ys = np.array([0.3], np.float32), np.array([1.4], np.float32)
    for H, bias in ((16, True), (8, False), (10, True)):
        h, W, b, y, t64, t32 = _case(ft, d, H, 513, seed=H, bias=bias)
        bb = None if b is None else torch.from_numpy(b).cuda()
        out, _ = ops.chain_log_prob_dense(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(),
                                          torch.from_numpy(W).cuda(), bb, ft, d, True, ym, ys)
        ref64 = O.log_pdf(y, t64, ft, d, True, ym, ys, np.float64)
        ref32 = O.log_pdf(y, t32, ft, d, True, ym, ys, np.float32)
        check_forward(out.cpu().numpy(), ref64, ref32, f"dense normalised H={H} bias={bias}", kind="dense")


def _post_case(ft, d, H, B, S, seed, shared_h=False, bias=True):
    rng = np.random.default_rng(seed)
    P = O.total_param_size(ft, d, True)
    h = rng.standard_normal((B, H) if shared_h else (S, B, H)).astype(np.float32)
    W = (rng.standard_normal((S, H, P)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal((S, P))).astype(np.float32) if bias else None
    y = rng.standard_normal((B, d)).astype(np.float32)
    hd = np.broadcast_to(h, (S, B, H)) if shared_h else h
    t64 = np.matmul(hd.astype(np.float64), W.astype(np.float64)) + (0 if b is None else b.astype(np.float64)[:, None])
    t32 = (np.matmul(hd, W) + (0 if b is None else b[:, None])).astype(np.float32)
    return h, W, b, y, t64, t32


@pytest.mark.parametrize("ft,d,H,B,S,shared", [
    (("planar", "radial") * 5, 1, 16, 1000, 8, False),   # the C5 chain (fused d = 1 kernel)
    (("planar", "radial") * 5, 1, 16, 777, 5, True),     # h shared by every draw (h draw stride 0)
    (("radial", "radial"), 1, 4, 333, 3, False),
    (("radial",) * 14, 1, 8, 301, 2, False),             # P = 44: three 16-column N tiles
    (("affine", "planar", "radial"), 3, 8, 300, 4, False),  # generic posterior kernel (d > 1)
    (("planar", "affine"), 8, 16, 129, 3, True),
    (("planar", "radial") * 2, 1, 32, 65, 1, False),     # S = 1
    (("radial", "planar") * 3 + ("radial",), 1, 16, 300, 3, False),  # odd alternating program
    (("planar",) * 3, 1, 8, 200, 2, False),
    # d >= 2, H <= 16, fast math: the prefetching posterior_densep_kernel (C3's flow stack at
    # d = 3, P = 60; a ragged last tile; h shared; H = 4)
    (("affine",) + ("planar",) * 4 + ("radial",) * 4, 3, 16, 777, 6, False),
    (("radial", "planar"), 2, 4, 65, 3, True),
    (("planar", "radial", "affine"), 4, 16, 1, 2, False),
])
def test_posterior_dense_matches_oracle(math_mode, ft, d, H, B, S, shared):
    """Bayesian posterior score with the output DenseVariational layer fused
    (BayesianNNEstimator.py:65-76, :136-145): against the oracle's posterior_lse on
    t_s = h_s W_s + b_s computed in fp64 (truth) / fp32 (the conditioning bound)."""
    from normalizingflownetwork_amd import ops

    h, W, b, y, t64, t32 = _post_case(ft, d, H, B, S, seed=H + B + S, shared_h=shared)
    out, s = ops.posterior_lse_dense(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(),
                                     torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), ft, d, True,
                                     want_sum=True)
    ref64 = O.posterior_lse(y, t64, ft, d, True, dtype=np.float64)
    ref32 = O.posterior_lse(y, t32, ft, d, True, dtype=np.float32)
    got = out.cpu().numpy()
    ok = np.isfinite(ref64)
    check_forward(got, ref64, ref32, f"posterior dense {ft[:2]}x{len(ft)} d={d} H={H} S={S} shared={shared} "
                  f"[{math_mode}]", nonfinite="match", kind="dense")
    bound = O.tolerance_bound(ref64, ref32)
    assert abs(s.item() - ref64[ok].sum()) <= bound[ok].sum() + 1e-6 * abs(ref64[ok].sum()) or not ok.all()


def test_posterior_dense_normalised_nobias_and_fallback(gpu):
    """y normalisation fused, no bias, and the unsupported-shape fallback (H = 12:
    library GEMM + posterior kernel) — all against the oracle."""
    from normalizingflownetwork_amd import ops

    ft, d, S = ("planar", "radial") * 3, 1, 4
    ym, ys = np.array([0.3], np.float32), np.array([1.4], np.float32)
    for H, bias in ((16, False), (12, True)):
        h, W, b, y, t64, t32 = _post_case(ft, d, H, 257, S, seed=7 + H, bias=bias)
        bb = None if b is None else torch.from_numpy(b).cuda()
        out, _ = ops.posterior_lse_dense(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(),
                                         torch.from_numpy(W).cuda(), bb, ft, d, True, ym, ys)
        ref64 = O.posterior_lse(y, t64, ft, d, True, ym, ys, np.float64)
        ref32 = O.posterior_lse(y, t32, ft, d, True, ym, ys, np.float32)
        check_forward(out.cpu().numpy(), ref64, ref32, f"posterior dense normalised H={H} bias={bias}", kind="dense")


@pytest.mark.parametrize("ft,d,H,B,bias,norm,mode", [
    (("radial",) * 14, 1, 8, 64 * 2 + 5, True, False, "fast"),          # P = 44: three N tiles, ragged last tile
    (("radial", "radial"), 1, 4, 65, False, False, "fast"),              # no bias
    (("planar", "radial") * 2, 1, 32, 64, True, True, "fast"),           # y normalisation
    (("affine", "planar", "radial"), 3, 8, 70, True, False, "fast"),     # posterior_densep_kernel
    (("affine", "planar", "radial"), 3, 8, 70, True, False, "precise"),  # posterior_dense_kernel
    (("radial", "planar"), 2, 4, 1, True, False, "fast"),
])
def test_posterior_dense_single_draw_is_bitwise_the_forward(gpu, ft, d, H, B, bias, norm, mode):
    """With one draw the posterior score is log_prob + log 1 - log 1, and the posterior kernels
    form t with the forward kernels' MFMA order and run the same chain evaluators: value for
    value (NaN matching NaN) posterior_lse_dense is chain_log_prob_dense, and so is the batch
    sum.  A guard against the copies of the tile pipeline drifting apart.  (d = 1, H = 16, P <= 32 in fast math is left out: there the forward forms t on
    split bf16 and the posterior on f32 MFMA, different by design.)"""
    from normalizingflownetwork_amd import ops

    h, W, b, y, _, _ = _case(ft, d, H, B, seed=H + B + d, bias=bias)
    ym = np.linspace(0.3, 0.5, d).astype(np.float32) if norm else None
    ys = np.linspace(1.4, 1.7, d).astype(np.float32) if norm else None
    yt, ht, Wt = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(), torch.from_numpy(W).cuda()
    bt = None if b is None else torch.from_numpy(b).cuda()
    prev = ops.set_math_mode(mode)
    try:
        fwd, fsum = ops.chain_log_prob_dense(yt, ht, Wt, bt, ft, d, True, ym, ys, want_sum=True)
        post, psum = ops.posterior_lse_dense(yt, ht, Wt[None], None if bt is None else bt[None], ft, d, True, ym, ys,
                                             want_sum=True)
    finally:
        ops.set_math_mode(prev)
    fwd, post = fwd.cpu().numpy(), post.cpu().numpy()
    assert fwd.shape == post.shape == (B,)
    same = (fwd.view(np.uint32) == post.view(np.uint32)) | (np.isnan(fwd) & np.isnan(post))
    assert same.all(), f"{(~same).sum()} of {B} values differ, first at {np.flatnonzero(~same)[:4]}"
    assert np.array_equal(np.float64(fsum.item()), np.float64(psum.item()), equal_nan=True)


def test_dense_full_size_c2_sampled(gpu):
    """The fused Dense forward at the C2 batch (2^24 rows, H = 16: the split-bf16 t GEMM) on
    y / h with the bench's scale: 65,536 random rows against the oracle on t = h W + b (the
    fp32 sensitivity widening as everywhere), every value finite, and the fused fp64 sum equal
    to the sum of the returned values."""
    from normalizingflownetwork_amd import ops

    ft, d, B, H = ("planar", "radial") * 5, 1, 1 << 24, 16
    P = O.total_param_size(ft, d, True)
    gen = torch.Generator(device="cuda").manual_seed(24)
    h = torch.randn((B, H), generator=gen, device="cuda")
    W = torch.randn((H, P), generator=gen, device="cuda") / 4.0
    b = 0.1 * torch.randn((P,), generator=gen, device="cuda")
    y = torch.randn((B, d), generator=gen, device="cuda")
    out, s = ops.chain_log_prob_dense(y, h, W, b, ft, d, True, want_sum=True)
    assert torch.isfinite(out).all()
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(3))[:1 << 16].cuda()
    hs, Wn, bn, ys = h[idx].cpu().numpy(), W.cpu().numpy(), b.cpu().numpy(), y[idx].cpu().numpy()
    t64 = hs.astype(np.float64) @ Wn.astype(np.float64) + bn.astype(np.float64)
    t32 = (hs @ Wn + bn).astype(np.float32)
    ref64 = O.chain_log_prob(ys, t64, ft, d, True, np.float64)
    ref32 = O.chain_log_prob(ys, t32, ft, d, True, np.float32)
    check_forward(out[idx].cpu().numpy(), ref64, ref32, "dense C2 full batch (65536 random rows)", kind="dense",
                  sensitivity=fp32_sensitivity(ys, t32, ft, d, True))
    assert abs(s.item() - out.double().sum().item()) <= 1e-9 * abs(s.item()) + 1e-6


def test_posterior_dense_full_size_c5_sampled(gpu):
    """C5 per-GPU shape (S = 64 draws x B = 2^17, H = 16): the fused kernel equals the
    unfused path (t_s materialised by the library GEMM, then the posterior kernel)
    within the fp32 GEMM-rounding bound, and sampled rows match the oracle."""
    from normalizingflownetwork_amd import ops

    ft, d, S, B, H = ("planar", "radial") * 5, 1, 64, 1 << 17, 16
    P = O.total_param_size(ft, d, True)
    gen = torch.Generator(device="cuda").manual_seed(5)
    h = torch.randn((S, B, H), generator=gen, device="cuda")
    W = torch.randn((S, H, P), generator=gen, device="cuda") / 4.0
    b = 0.1 * torch.randn((S, P), generator=gen, device="cuda")
    y = torch.randn((B, d), generator=gen, device="cuda")
    out, s = ops.posterior_lse_dense(y, h, W, b, ft, d, True, want_sum=True)
    assert torch.isfinite(out).all()
    idx = torch.randperm(B, generator=torch.Generator().manual_seed(2))[:256]
    hs, Ws, bs = h[:, idx.cuda()].cpu().numpy(), W.cpu().numpy(), b.cpu().numpy()
    t64 = np.matmul(hs.astype(np.float64), Ws.astype(np.float64)) + bs.astype(np.float64)[:, None]
    t32 = (np.matmul(hs, Ws) + bs[:, None]).astype(np.float32)
    ys = y[idx.cuda()].cpu().numpy()
    ref64 = O.posterior_lse(ys, t64, ft, d, True, dtype=np.float64)
    ref32 = O.posterior_lse(ys, t32, ft, d, True, dtype=np.float32)
    got = out[idx.cuda()].cpu().numpy()
    check_forward(got, ref64, ref32, "posterior dense C5 sample", kind="dense")
    assert abs(s.item() - out.double().sum().item()) <= 1e-9 * abs(s.item()) + 1e-6


@pytest.mark.parametrize("ft,d,H,B", [(("planar", "radial") * 5, 1, 16, 1000), (("radial", "radial"), 1, 4, 333),
                                      (("affine", "planar", "radial"), 3, 8, 300), (("planar", "affine"), 8, 16, 129),
                                      (("radial",) * 14, 1, 32, 201),
                                      # the estimator's default radial x 10 at H = 16: a cached compile-time program
                                      (("radial",) * 10, 1, 16, 777),
                                      # odd alternating / homogeneous programs (hpair_types)
                                      (("planar", "radial") * 3 + ("planar",), 1, 16, 500),
                                      (("radial", "planar") * 2 + ("radial",), 1, 8, 300),
                                      (("planar",) * 5, 1, 4, 257)])
def test_dense_grad_matches_oracle(math_mode, ft, d, H, B):
    """Backward through the fused output Dense layer + chain (nfn_chain_logprob_dense_grad_f32):
    dL/dh = dt W^T, dL/dW = h^T dt, dL/db = sum dt, dL/dy — against the autodiff oracle's dt
    (fp64, at the fp32 t) pushed through the same products in fp64.  Bounds: the oracle's
    per-element dt tolerance carried through |W| / |h|, plus 1e-5 of the products' magnitudes
    (fp32 MFMA accumulation)."""
    from oracle import nfn_grad_oracle as G
    from normalizingflownetwork_amd import ops

    h, W, b, y, t64, t32 = _case(ft, d, H, B, seed=3 * H + B)
    rng = np.random.default_rng(B)
    g = rng.standard_normal(B).astype(np.float32)
    lp, gh, gW, gb, gy = ops.chain_log_prob_dense_grad(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(),
                                                       torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), ft, d,
                                                       True, g_out=torch.from_numpy(g).cuda(), want_logp=True)
    gt64, gy64, dev_t, dev_y = G.fp32_spread(y, t32, ft, d, True, g_out=g)
    bt = G.grad_tolerance(gt64, dev_t)
    fin = np.isfinite(gt64).all(1)
    assert fin.all(), "oracle non-finite on this case"
    W64, h64 = W.astype(np.float64), h.astype(np.float64)
    gh_ref, gW_ref, gb_ref = gt64 @ W64.T, h64.T @ gt64, gt64.sum(0)
    bh = bt @ np.abs(W64).T + 1e-5 * (np.abs(gt64) @ np.abs(W64).T) + 1e-7
    bW = np.abs(h64).T @ bt + 1e-5 * (np.abs(h64).T @ np.abs(gt64)) + 1e-6
    bb = bt.sum(0) + 1e-5 * np.abs(gt64).sum(0) + 1e-6
    for got, ref, bound, what in ((gh, gh_ref, bh, "dh"), (gW, gW_ref, bW, "dW"), (gb, gb_ref, bb, "db")):
        check_bound(got.cpu().numpy(), ref, bound, f"dense grad {what} {ft[:2]}x{len(ft)} d={d} H={H} [{math_mode}]",
                    kind="dense_grad")
    check_grad(gy.cpu().numpy(), gy64, dev_y, f"dense grad dy {ft[:2]}x{len(ft)} d={d} H={H} [{math_mode}]")
    ref64 = O.chain_log_prob(y, t64, ft, d, True, np.float64)
    ref32 = O.chain_log_prob(y, t32, ft, d, True, np.float32)
    check_forward(lp.cpu().numpy(), ref64, ref32, f"dense grad log_prob {ft[:2]}x{len(ft)} d={d} H={H} [{math_mode}]",
                  kind="dense_grad", sensitivity=fp32_sensitivity(y, t32, ft, d, True))
    # deterministic: a second run is bitwise identical
    _, gh2, gW2, gb2, _ = ops.chain_log_prob_dense_grad(torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(),
                                                         torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), ft,
                                                         d, True, g_out=torch.from_numpy(g).cuda())
    assert torch.equal(gh, gh2) and torch.equal(gW, gW2) and torch.equal(gb, gb2)


def test_dense_grad_full_size_against_oracle(gpu):
    """The fused Dense backward at the C2 batch (2^24 rows, H = 16), against the oracles:
    * dh and dy on 4,096 random rows: the autodiff oracle (fp64) at the rows' fp32 t, with
      grad_tolerance's per-element bound (the fp32 autodiff spread) carried through |W| as in
      test_dense_grad_matches_oracle;
    * dW and db (sums over all 2^24 rows): the closed-form fp64 reverse pass
      (tests/analytic_grad.py, itself pinned to the autodiff oracle by test_grad_oracle) over
      every row, summed in fp64; per row the bound is grad_tolerance with the fp32 runs of the
      same closed form at the inputs and at two 1-ulp perturbations as the spread (as
      nfn_grad_oracle.fp32_spread), summed through |h| like the products, plus 1e-5 of the
      products' magnitudes (fp32 MFMA accumulation over 2^24 rows).  With N(0, 1)-scale t the
      gradients are heavy-tailed (dt up to ~1e11 near the flows' singular parameters, e.g.
      planar w -> 0): the 0.5 % of rows with entries above 1e6 carry essentially all of
      sum |dt|, so they set both the sums and their bounds.  dW and db are therefore ALSO
      checked on a second launch whose upstream gradient is zero on every row with an oracle
      gradient entry above 100 in magnitude (their dt, hence their share of dW and db, is
      then exactly 0): the remaining rows' sums against the oracle's over the same rows,
      where the bound is a few % of the sums instead of orders of magnitude above them.
    h, W and b sit on dyadic grids that make t = h W + b exact in fp32, so kernel and oracle
    evaluate the chain at the same t.
    The upstream gradient is N(0, 1) per row (unit scale, so the 2e-5 floor is not slack)."""
    from concurrent.futures import ThreadPoolExecutor

    import analytic_grad as A
    from oracle import nfn_grad_oracle as G
    from normalizingflownetwork_amd import ops

    ft, d = ("planar", "radial") * 5, 1
    P = O.total_param_size(ft, d, True)
    B, H = 1 << 24, 16
    gen = torch.Generator(device="cuda").manual_seed(9)
    # h, W, b on coarse dyadic grids (multiples of 1/8, 1/64, 1/64): every product and
    # partial sum of t = h W + b is exact in fp32, so the matrix cores' t IS numpy's and the
    # oracle's (near a singular parameter the chain would otherwise amplify their different
    # roundings by orders of magnitude: no bound then separates kernel error from input noise)
    h = torch.randint(-8, 9, (B, H), generator=gen, device="cuda").float() / 8.0
    W = torch.randint(-16, 17, (H, P), generator=gen, device="cuda").float() / 64.0
    b = torch.randint(-8, 9, (P,), generator=gen, device="cuda").float() / 64.0
    y = torch.randn((B, d), generator=gen, device="cuda")
    g = torch.randn((B,), generator=gen, device="cuda")
    _, gh, gW, gb, gy = ops.chain_log_prob_dense_grad(y, h, W, b, ft, d, True, g_out=g)
    hn, Wn, bn, yn, gn = (x.cpu().numpy() for x in (h, W, b, y, g))
    ghn, gyn = gh.cpu().numpy(), gy.cpu().numpy()
    W64 = Wn.astype(np.float64)
    rng = np.random.default_rng(4096)
    idx = np.sort(rng.choice(B, 4096, replace=False))
    t32 = (hn[idx] @ Wn + bn).astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), hn[idx].astype(np.float64) @ W64 + bn.astype(np.float64))
    gt64, gy64, dev_t, dev_y = G.fp32_spread(yn[idx], t32, ft, d, True, g_out=gn[idx])
    bt = G.grad_tolerance(gt64, dev_t)
    check_bound(ghn[idx], gt64 @ W64.T, bt @ np.abs(W64).T + 1e-5 * (np.abs(gt64) @ np.abs(W64).T) + 1e-7,
                "dense grad dh C2 full batch (4096 random rows)", kind="dense_grad")
    check_grad(gyn[idx], gy64, dev_y, "dense grad dy C2 full batch (4096 random rows)")

    # Only elementwise numpy runs in the worker threads (the closed form's per-row math):
    # concurrent BLAS calls from several Python threads corrupted whole rows of the chunk
    # matmuls in an earlier form of this test, so every product is formed here, serially.
    h64 = hn.astype(np.float64)
    T = (h64 @ W64 + bn.astype(np.float64)).astype(np.float32)  # exact (dyadic grids)
    G64 = np.empty((B, P), np.float64)
    BT = np.empty((B, P), np.float64)
    EPS = np.empty((B, P), np.float32)  # per-element dt error model of the well-conditioned rows
    GOOD = np.empty((B,), bool)

    def chunk(lo):
        hi = min(B, lo + (1 << 20))
        gc = gn[lo:hi].astype(np.float64)[:, None]
        tc, yc = T[lo:hi], yn[lo:hi]
        prng = np.random.default_rng(lo)
        with np.errstate(all="ignore"):
            _, g64, _ = A.chain_grad(yc, tc, ft, d, True, dtype=np.float64)
            g64 = g64 * gc
            # the fp32 spread as nfn_grad_oracle.fp32_spread builds it: the fp32 run at the
            # inputs and at two 1-ulp perturbations of them
            dev = np.zeros_like(g64)
            for k in range(3):
                tk, yk = tc, yc
                if k:
                    tk = (tc * (1 + prng.integers(-1, 2, tc.shape) * 2.0 ** -23)).astype(np.float32)
                    yk = (yc * (1 + prng.integers(-1, 2, yc.shape) * 2.0 ** -23)).astype(np.float32)
                _, g32, _ = A.chain_grad(yk, tk, ft, d, True, dtype=np.float32)
                dev = np.maximum(dev, np.abs(g32.astype(np.float64) * gc - g64))
        G64[lo:hi] = g64
        BT[lo:hi] = G.grad_tolerance(g64, dev)
        rmax = np.abs(g64).max(axis=1)
        GOOD[lo:hi] = (rmax <= 1.0) & (dev.max(axis=1) <= 1e-6 * rmax)
        EPS[lo:hi] = 8.0 * dev + 2.0 ** -20 * rmax[:, None]

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(chunk, range(0, B, 1 << 20)))
    assert np.isfinite(G64).all(), "closed-form oracle non-finite on this batch"
    ha = np.abs(h64)
    # the heavy tail that dominates the sums: rows with an oracle gradient entry above 100
    ill_mask = np.abs(G64).max(axis=1) > 100.0
    wc = ~ill_mask
    ill = np.flatnonzero(ill_mask)
    W_ref, bW = h64.T @ G64, ha.T @ BT + 1e-5 * (ha.T @ np.abs(G64))
    b_ref, bb = G64.sum(0), BT.sum(0) + 1e-5 * np.abs(G64).sum(0)
    W_wc, bW_wc = h64[wc].T @ G64[wc], ha[wc].T @ BT[wc] + 1e-5 * (ha[wc].T @ np.abs(G64[wc]))
    b_wc, bb_wc = G64[wc].sum(0), BT[wc].sum(0) + 1e-5 * np.abs(G64[wc]).sum(0)
    check_bound(gW.cpu().numpy(), W_ref, bW + 1e-6, "dense grad dW C2 full batch (2^24 rows)", kind="dense_grad")
    check_bound(gb.cpu().numpy(), b_ref, bb + 1e-6, "dense grad db C2 full batch (2^24 rows)", kind="dense_grad")
    assert ill.size < B // 5, f"{ill.size} rows with gradient entries above 100"
    g_wc = g.clone()
    g_wc[torch.from_numpy(ill).cuda()] = 0.0
    _, _, gW2, gb2, _ = ops.chain_log_prob_dense_grad(y, h, W, b, ft, d, True, g_out=g_wc)
    check_bound(gW2.cpu().numpy(), W_wc, bW_wc + 1e-6,
                f"dense grad dW C2 full batch, the {B - ill.size} rows with |dt| <= 100", kind="dense_grad")
    check_bound(gb2.cpu().numpy(), b_wc, bb_wc + 1e-6,
                f"dense grad db C2 full batch, the {B - ill.size} rows with |dt| <= 100", kind="dense_grad")

    # A bound that can fail (verdict r04): the well-conditioned rows only — every oracle dt
    # entry at most 1 and the row's fp32 spread at most 1e-6 of its largest entry — with an
    # error MODEL instead of the summed per-row tolerance.  Both terms are random-sign sums
    # (statistical, not worst-case; 8 standard deviations):
    #  * fp32 accumulation: each wave sums its tiles' h^T dt in MFMA accumulators, 16 steps per
    #    64-row tile over at most ceil(tiles / 256) tiles (a launch runs >= 256 waves): error
    #    ~ 2^-24 sqrt(depth) |partial sums| ~ 2^-24 sqrt(depth) sqrt(sum_b (h_b dt_b)^2);
    #  * the kernel's per-row dt error, at most EPS = 8 x the fp32 spread + 2^-20 x the row's
    #    largest entry per element, summed through h: sqrt(sum_b h_b^2 EPS_b^2).
    # The rows outside the set get a zero upstream gradient (their dt, hence their share, is
    # exactly 0).  A negative control then zeroes ONE 256-row block of the set in the kernel's
    # input only: the check must trip.
    good = np.flatnonzero(GOOD)
    assert good.size > B // 4, f"only {good.size} well-conditioned rows"
    mask_dev = torch.zeros((B,), dtype=torch.bool, device="cuda")
    mask_dev[torch.from_numpy(good).cuda()] = True
    g_good = torch.where(mask_dev, g, torch.zeros_like(g))
    _, _, gW3, gb3, _ = ops.chain_log_prob_dense_grad(y, h, W, b, ft, d, True, g_out=g_good)
    Hg, Gg, Eg = h64[good], G64[good], EPS[good].astype(np.float64)
    W_g, b_g = Hg.T @ Gg, Gg.sum(0)
    depth = 16 * -(-(B // 64) // 256)
    acc = 2.0 ** -24 * np.sqrt(depth)
    H2 = Hg * Hg
    bW_g = 8.0 * (acc * np.sqrt(H2.T @ (Gg * Gg)) + np.sqrt(H2.T @ (Eg * Eg)))
    bb_g = 8.0 * (acc * np.sqrt((Gg * Gg).sum(0)) + np.sqrt((Eg * Eg).sum(0)))
    rW = check_bound(gW3.cpu().numpy(), W_g, bW_g,
                     f"dense grad dW C2 full batch, the {good.size} well-conditioned rows (error model)",
                     kind="dense_grad")
    rb = check_bound(gb3.cpu().numpy(), b_g, bb_g,
                     f"dense grad db C2 full batch, the {good.size} well-conditioned rows (error model)",
                     kind="dense_grad")
    print(f"well-conditioned dW / db: max err / bound {rW:.3g} / {rb:.3g} over {good.size} rows")
    # negative control: the 256-row block (of the set) that carries the largest sum |h dt|
    contrib = np.zeros(B // 256)
    np.add.at(contrib, good // 256, np.abs(Hg).sum(1) * np.abs(Gg).sum(1))
    blk = int(np.argmax(contrib))
    g_neg = g_good.clone()
    g_neg[blk * 256:(blk + 1) * 256] = 0.0
    _, _, gW4, gb4, _ = ops.chain_log_prob_dense_grad(y, h, W, b, ft, d, True, g_out=g_neg)
    errW = np.abs(gW4.cpu().numpy().astype(np.float64) - W_g) / bW_g
    errb = np.abs(gb4.cpu().numpy().astype(np.float64) - b_g) / bb_g
    assert max(errW.max(), errb.max()) > 1.0, \
        f"negative control (block {blk} of 256 rows dropped) passed the bound: {errW.max():.3g} / {errb.max():.3g}"
    print(f"negative control (block {blk} dropped): max err / bound {errW.max():.3g} (dW) / {errb.max():.3g} (db)")


def test_dense_grad_fallback_matches_unfused(gpu):
    """The unfused fallback (H = 12: library GEMM t + chain backward kernel + library GEMMs)
    gives the fused formulas' dW."""
    from normalizingflownetwork_amd import ops

    ft, d = ("planar", "radial") * 5, 1
    P = O.total_param_size(ft, d, True)
    gen = torch.Generator(device="cuda").manual_seed(9)
    b = 0.1 * torch.randn((P,), generator=gen, device="cuda")
    y = torch.randn((300, d), generator=gen, device="cuda")
    h12 = torch.randn((300, 12), generator=gen, device="cuda")
    W12 = torch.randn((12, P), generator=gen, device="cuda") / 4.0
    _, gh12, gW12, gb12, _ = ops.chain_log_prob_dense_grad(y, h12, W12, b, ft, d, True)
    _, gt12, _ = ops.chain_log_prob_grad(y, h12 @ W12 + b, ft, d, True)
    torch.testing.assert_close(gW12, h12.t() @ gt12)


@pytest.mark.parametrize("ft,H,B,trainable,g_none", [
    (("planar", "radial") * 5, 16, 64 * 37 + 5, True, False),
    (("affine", "planar", "radial", "affine"), 16, 640, False, True),
    (("radial", "planar") * 3 + ("affine",), 32, 64 * 9 + 63, True, True),
    (("planar",) * 16, 32, 77, False, False),
    (("radial",), 16, 1, True, False),
    # the cached compile-time programs (C2's with a fixed base, the estimator's radial x 10)
    (("planar", "radial") * 5, 16, 200, False, True),
    (("radial",) * 10, 16, 64 * 5 + 17, True, True)])
def test_dense1_grad_kernel_shapes(gpu, ft, H, B, trainable, g_none):
    """The d = 1 fast-math fused Dense backward (chain_dense1_grad_kernel: H in {16, 32},
    P <= 64) over ragged batches, widths P not a multiple of 16, a fixed base, a missing
    upstream gradient (= ones) and y normalisation (mean 0.25, std 2: the kernel's
    (y - m) / s is then bitwise numpy's), against the autodiff oracle as above."""
    from oracle import nfn_grad_oracle as G
    from normalizingflownetwork_amd import ops

    d = 1
    rng = np.random.default_rng(B + H)
    P = O.total_param_size(ft, d, trainable)
    h = rng.standard_normal((B, H)).astype(np.float32)
    W = (rng.standard_normal((H, P)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(P)).astype(np.float32)
    y = rng.standard_normal((B, d)).astype(np.float32)
    t32 = (h @ W + b).astype(np.float32)
    g = None if g_none else rng.standard_normal(B).astype(np.float32)
    ym, ys = np.float32(0.25), np.float32(2.0)
    z = ((y - ym) / ys).astype(np.float32)
    lp, gh, gW, gb, gy = ops.chain_log_prob_dense_grad(
        torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(),
        ft, d, trainable, y_mean=torch.tensor([ym]).cuda(), y_std=torch.tensor([ys]).cuda(),
        g_out=None if g is None else torch.from_numpy(g).cuda(), want_logp=True)
    gg = np.ones(B, np.float32) if g is None else g
    gt64, gy64, dev_t, dev_y = G.fp32_spread(z, t32, ft, d, trainable, g_out=gg)
    bt = G.grad_tolerance(gt64, dev_t)
    assert np.isfinite(gt64).all()
    W64, h64 = W.astype(np.float64), h.astype(np.float64)
    gh_ref, gW_ref, gb_ref = gt64 @ W64.T, h64.T @ gt64, gt64.sum(0)
    bh = bt @ np.abs(W64).T + 1e-5 * (np.abs(gt64) @ np.abs(W64).T) + 1e-7
    bW = np.abs(h64).T @ bt + 1e-5 * (np.abs(h64).T @ np.abs(gt64)) + 1e-6
    bb = bt.sum(0) + 1e-5 * np.abs(gt64).sum(0) + 1e-6
    for got, ref, bound, what in ((gh, gh_ref, bh, "dh"), (gW, gW_ref, bW, "dW"), (gb, gb_ref, bb, "db")):
        check_bound(got.cpu().numpy(), ref, bound, f"dense1 grad {what} {ft[:2]}x{len(ft)} H={H} B={B}",
                    kind="dense_grad")
    check_grad(gy.cpu().numpy(), gy64 / 2.0, dev_y / 2.0, f"dense1 grad dy {ft[:2]}x{len(ft)} H={H} B={B}")
    t64 = h64 @ W64 + b.astype(np.float64)
    ref64 = O.chain_log_prob(z, t64, ft, d, trainable, np.float64) - np.log(2.0)
    ref32 = O.chain_log_prob(z, t32, ft, d, trainable, np.float32) - np.float32(np.log(2.0))
    sens = fp32_sensitivity(z, t32, ft, d, trainable)
    check_forward(lp.cpu().numpy(), ref64, ref32, f"dense1 grad log_prob {ft[:2]}x{len(ft)} H={H} B={B}",
                  kind="dense_grad", sensitivity=sens)
