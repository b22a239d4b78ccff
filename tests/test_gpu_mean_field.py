"""The fused mean-field kernels on the GPU (nfn_meanfield.hip: nfn_mean_field_draw_kl_f32 and
its backward) against the fp64 oracle (tests/mean_field_oracle.py), and the autograd op.

Sizes sit where the kernels can go wrong: below one group of four (1, 3), around a wave (63, 64,
65) and a workgroup's 4 x 256 elements (255, 257, 1023), several workgroups with a ragged tail
(4099, 70 001), and one vector longer than the capped grid covers in one pass (2^21 + 4099: the
grid-stride loop runs twice).  ``loc``, ``rho``, ``eps`` and ``g_w`` are views at four different
element offsets 0-3 of larger buffers, rotated from one prior setting to the next, so ``loc``
(whose alignment places the groups) takes every phase and the other arrays take both the
16-byte and the dword path.

Gate (README "Parity"): every element of ``w`` and of each gradient within ``1e-5 max(1, |ref64|)``
of the fp64 oracle at the same fp32 inputs, or within 2x the fp32 mirror's own error on that
element — the latter for at most 1 % of a case's elements (tests/test_mean_field_oracle.py shows
the mirror itself leaves the plain bound on fewer).  The KL sum is assembled in fp64 and gets no
widening."""

import numpy as np
import pytest
import torch

from conftest import WIDEN_CAP, record_parity
from normalizingflownetwork_amd import ops

import mean_field_oracle as MF

pytestmark = pytest.mark.gpu

BASE = 1e-5
WIDEN_SHARE = 0.01
SIZES = [1, 3, 63, 64, 65, 255, 257, 1023, 4099, 70001]
LONG = (1 << 21) + 4099
PRIOR_SCALES = (0.1, 1.0, 10.0)
G_KL = 0.7
MODES = [(True, False), (False, False), (True, True), (False, True)]  # (kl_exact, map mode)


def seed_of(N):
    return N


def _view(a, offset):
    """``a`` on the device as a view at element ``offset`` of a larger, NaN-filled buffer."""
    if a is None:
        return None
    buf = torch.full((a.size + 8,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + a.size] = torch.as_tensor(a, device="cuda")
    return buf[offset:offset + a.size]


def _gate(what, got, ref64, ref32, widen=True, kind="forward"):
    got, ref64, ref32 = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape, what
    assert np.isfinite(ref64).all() and np.isfinite(got).all(), what
    err = np.abs(got - ref64)
    base = BASE * np.maximum(1.0, np.abs(ref64))
    wide = WIDEN_CAP * np.abs(ref32 - ref64) if widen else np.zeros_like(base)
    bound = np.maximum(base, wide)
    record_parity(what, got, ref64, ref32, err, bound, kind=kind)
    n_wide = int((err > base).sum())
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}, max err / plain bound = "
          f"{float((err / base).max()) if err.size else 0.0:.3f}, {n_wide} of {err.size} beyond the plain bound")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the bound"
    assert n_wide <= int(WIDEN_SHARE * err.size), f"{what}: {n_wide} of {err.size} pass only by the widening"


def _run_case(N, kl_exact, map_mode, prior, ps, k, seed=None):
    tag = f"N={N} {'exact' if kl_exact else 'sampled'} {'map' if map_mode else 'full'} prior={prior} sp={ps}"
    loc, rho, eps, g_w, p = MF.make_inputs(N, seed_of(N) if seed is None else seed, prior)
    if map_mode:
        rho = eps = None
    d_loc, d_rho, d_eps, d_gw = (_view(a, (k + j) % 4) for j, a in enumerate((loc, rho, eps, g_w)))
    d_p = _view(p, (k + 1) % 4)
    g_kl = torch.tensor([G_KL], device="cuda")
    w, kl = ops.mean_field_draw_kl(d_loc, d_rho, d_eps, d_p, ps, kl_exact)
    gl, gr, gp = ops.mean_field_draw_kl_grad(d_loc, d_rho, d_eps, d_p, ps, kl_exact, g_w=d_gw, g_kl=g_kl,
                                             want_grad_prior=True)
    torch.cuda.synchronize()
    w64, kl64 = MF.draw_kl(loc, rho, eps, p, ps, kl_exact)
    w32, kl32 = MF.draw_kl(loc, rho, eps, p, ps, kl_exact, dtype=torch.float32)
    if map_mode:
        assert torch.equal(w, d_loc) and gr is None
    _gate(f"{tag} w", w.cpu().numpy(), w64, w32)
    kl = kl.cpu().numpy()
    assert kl[1] == 0.0
    _gate(f"{tag} kl", kl[0], kl64, kl32, widen=False)
    r64 = MF.draw_kl_grads(loc, rho, eps, p, ps, kl_exact, g_w, G_KL)
    r32 = MF.draw_kl_grads(loc, rho, eps, p, ps, kl_exact, g_w, G_KL, dtype=torch.float32)
    for name, got, a, b in zip(("grad_loc", "grad_rho", "grad_prior_loc"), (gl, gr, gp), r64, r32):
        if a is not None:
            _gate(f"{tag} {name}", got.cpu().numpy(), a, b, kind="backward")
    # the KL alone (no w written) and the draw alone give the same numbers
    _, kl_only = ops.mean_field_draw_kl(d_loc, d_rho, d_eps, d_p, ps, kl_exact, want_w=False)
    w_only, none = ops.mean_field_draw_kl(d_loc, d_rho, d_eps, d_p, ps, kl_exact, want_kl=False)
    assert none is None and torch.equal(w_only, w) and np.array_equal(kl_only.cpu().numpy(), kl)


@pytest.mark.parametrize("kl_exact,map_mode", MODES)
@pytest.mark.parametrize("N", SIZES)
def test_parity(gpu, N, kl_exact, map_mode):
    k = 0
    for prior in (False, True):
        for ps in PRIOR_SCALES:
            _run_case(N, kl_exact, map_mode, prior, ps, k)
            k += 1


def test_parity_beyond_one_pass_of_the_grid(gpu):
    _run_case(LONG, True, False, True, 1.0, 1, seed=1)
    _run_case(LONG, False, False, False, 0.1, 2, seed=2)


def test_empty_vector(gpu):
    e = torch.empty((0,), device="cuda")
    for rho, eps in ((e, e), (None, None)):
        w, kl = ops.mean_field_draw_kl(e, rho, eps)
        assert w.numel() == 0 and kl.cpu().tolist() == [0.0, 0.0]
        gl, gr, gp = ops.mean_field_draw_kl_grad(e, rho, eps, g_kl=torch.ones(1, device="cuda"))
        assert gl.numel() == 0 and gp is None


def _dev_inputs(N, seed, prior=True):
    return [None if a is None else torch.as_tensor(a, device="cuda") for a in MF.make_inputs(N, seed, prior)]


@pytest.mark.parametrize("kl_exact", [True, False])
def test_kl_is_bitwise_deterministic_and_needs_no_workspace_initialisation(gpu, kl_exact):
    N = 70001
    loc, rho, eps, _, p = _dev_inputs(N, 11)
    first = ops.mean_field_draw_kl(loc, rho, eps, p, 1.0, kl_exact)[1].cpu().numpy()
    again = ops.mean_field_draw_kl(loc, rho, eps, p, 1.0, kl_exact)[1].cpu().numpy()
    assert first.tobytes() == again.tobytes()
    ws = ops._workspace(int(ops._lib.load().nfn_mean_field_workspace_doubles(N)), loc.device)
    for fill in (255, 0):
        torch.cuda.synchronize()
        ws.view(torch.uint8).fill_(fill)
        got = ops.mean_field_draw_kl(loc, rho, eps, p, 1.0, kl_exact)[1].cpu().numpy()
        assert got.tobytes() == first.tobytes(), fill


@pytest.mark.parametrize("N,at", [(70001, 31337), (70001, 0), (70001, 70000), (3, 1)])
def test_a_nan_is_counted(gpu, N, at):
    loc, rho, eps, _, p = _dev_inputs(N, 13)
    loc[at] = float("nan")
    kl = ops.mean_field_draw_kl(loc, rho, eps, p)[1].cpu().numpy()
    assert np.isnan(kl[0]) and kl[1] == 1.0


@pytest.mark.parametrize("kl_exact,map_mode", MODES)
@pytest.mark.parametrize("prior", [False, True])
def test_autograd_op_matches_the_oracle(gpu, kl_exact, map_mode, prior):
    """``mean_field_draw_kl_diff`` under autograd against the oracle's autograd on N = 65, compared
    in fp32 under the parity rule (the op is fp32: this is not a literal fp64 ``gradcheck``)."""
    N, ps = 65, 0.5
    loc, rho, eps, g_w, p = MF.make_inputs(N, 17, prior)
    if map_mode:
        rho = eps = None
    leaves = [None if a is None else torch.as_tensor(a, device="cuda").requires_grad_(True) for a in (loc, rho, p)]
    d_eps = None if eps is None else torch.as_tensor(eps, device="cuda")
    w, kl = ops.mean_field_draw_kl_diff(leaves[0], leaves[1], d_eps, leaves[2], ps, kl_exact)
    assert kl.dtype == torch.float32 and kl.dim() == 0 and kl.is_cuda
    ((torch.as_tensor(g_w, device="cuda") * w).sum() + G_KL * kl).backward()
    w64, kl64 = MF.draw_kl(loc, rho, eps, p, ps, kl_exact)
    assert abs(kl.item() - kl64) <= BASE * max(1.0, abs(kl64))
    r64 = MF.draw_kl_grads(loc, rho, eps, p, ps, kl_exact, g_w, G_KL)
    r32 = MF.draw_kl_grads(loc, rho, eps, p, ps, kl_exact, g_w, G_KL, dtype=torch.float32)
    for name, leaf, a, b in zip(("loc", "rho", "prior_loc"), (leaves[0], leaves[1], leaves[2]), r64, r32):
        if leaf is not None:
            _gate(f"autograd {kl_exact} {map_mode} {prior} d{name}", leaf.grad.cpu().numpy(), a, b, kind="backward")
    # the KL alone: no gradient reaches the draw
    for leaf in leaves:
        if leaf is not None:
            leaf.grad = None
    ops.mean_field_draw_kl_diff(leaves[0], leaves[1], d_eps, leaves[2], ps, kl_exact)[1].backward()
    only_kl = MF.draw_kl_grads(loc, rho, eps, p, ps, kl_exact, None, 1.0)
    only_kl32 = MF.draw_kl_grads(loc, rho, eps, p, ps, kl_exact, None, 1.0, dtype=torch.float32)
    _gate("autograd kl only dloc", leaves[0].grad.cpu().numpy(), only_kl[0], only_kl32[0], kind="backward")
