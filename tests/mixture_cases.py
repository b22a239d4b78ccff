"""The two mixture layers behind one interface, and the checks that tests/test_gpu_mdn.py,
tests/test_gpu_kernel_mixture.py and tests/test_gpu_posterior_mixture.py share.

A case holds one seeded input set and knows its layer's ops and fp64 numpy oracles
(tests/mdn_oracle.py, tests/mixture_oracle.py, tests/posterior_mixture_oracle.py).  Its ``rows``
are (B, W) parameter rows for the forward and the gradients, or (S, B, W) draws for the
posterior score; ``op`` and ``ref`` take either.

Tolerance of every forward check: the project's base bound ``1e-5 * max(1, |ref64|)`` per
element plus exact agreement of the finite mask."""

import numpy as np
import torch

from conftest import record_parity
from normalizingflownetwork_amd import ops

import mdn_oracle as MD
import mixture_oracle as MO
import posterior_mixture_oracle as PO

BASE = 1e-5


def _dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float32), device="cuda")


def _norm(d):
    return np.linspace(-0.5, 0.5, d).astype(np.float32), np.linspace(0.5, 2.0, d).astype(np.float32)


class Gmm:
    """The Gaussian-mixture layer (nfn_gmm.hip): rows of P = K (2 d + 1) parameters."""

    grad_names = ("grad_t", "grad_y")

    def __init__(self, B, K, d, S=None, **scaling):
        """``S`` draws (tests/posterior_mixture_oracle.py's seeds), or one set of rows, where
        ``scaling`` may carry the ``seed`` of tests/mdn_oracle.py's ``make_inputs``."""
        self.K, self.d = K, d
        if S is None:
            self.y, self.rows = MD.make_inputs(B, K, d, **scaling)
            self.tag = f"gmm B={B} K={K} d={d}"
        else:
            self.y, self.rows = PO.make_gmm_inputs(S, B, K, d, **scaling)
            self.tag = f"gmm posterior B={B} S={S} K={K} d={d}"

    def op(self, y, rows, ym=None, ys=None, **want):
        f = ops.posterior_lse_gaussian_mixture if rows.dim() == 3 else ops.gaussian_mixture_log_prob
        return f(y, rows, self.K, self.d, ym, ys, **want)

    def ref(self, y, rows, ym=None, ys=None, dtype=np.float64):
        f = PO.gmm_posterior if np.ndim(rows) == 3 else MD.log_prob
        return f(y, rows, self.K, self.d, ym, ys, dtype)

    def grad(self, g, ym=None, ys=None):
        """``(logp, grad_t, grad_y)`` of the case's inputs under the upstream gradient ``g``."""
        out = ops.gaussian_mixture_log_prob_grad(_dev(self.y), _dev(self.rows), self.K, self.d, ym, ys, g_out=_dev(g),
                                                 want_logp=True)
        return [a.cpu().numpy() for a in out]

    def grad_ref(self, g, ym=None, ys=None, dtype=np.float64):
        """The oracle's arrays in ``grad_names`` order, and per array what conditions it (None:
        its own magnitude)."""
        return MD.log_prob_grads(self.y, self.rows, self.K, self.d, g, ym, ys, dtype), (None, None)

    def logits(self, rows):
        """The view of the logit columns of ``rows``."""
        return rows[..., 2 * self.K * self.d:]


class Kernel:
    """The kernel-mixture layer (nfn_mixture.hip): rows of M logits, centres and scales per case."""

    grad_names = ("grad_logits", "grad_y", "grad_scales")

    def __init__(self, B, M, d, S=None, **scaling):
        """As ``Gmm``: ``S`` draws, or one set of rows with an optional ``seed`` in ``scaling``."""
        self.M, self.d = M, d
        if S is None:
            self.y, self.rows, self.locs, self.scales = MO.make_inputs(B, M, d, **scaling)
            self.tag = f"kernel B={B} M={M} d={d}"
        else:
            self.y, self.rows, self.locs, self.scales = PO.make_kernel_inputs(S, B, M, d, **scaling)
            self.tag = f"kernel posterior B={B} S={S} M={M} d={d}"
        self.dl, self.ds = _dev(self.locs), _dev(self.scales)

    def op(self, y, rows, ym=None, ys=None, **want):
        f = ops.posterior_lse_kernel_mixture if rows.dim() == 3 else ops.kernel_mixture_log_prob
        return f(y, rows, self.dl, self.ds, ym, ys, **want)

    def ref(self, y, rows, ym=None, ys=None, dtype=np.float64):
        f = PO.kernel_posterior if np.ndim(rows) == 3 else MO.log_prob
        return f(y, rows, self.locs, self.scales, ym, ys, dtype)

    def grad(self, g, ym=None, ys=None):
        """``(logp, grad_logits, grad_y, grad_scales)``."""
        out = ops.kernel_mixture_log_prob_grad(_dev(self.y), _dev(self.rows), self.dl, self.ds, ym, ys, g_out=_dev(g),
                                               want_logp=True)
        return [a.cpu().numpy() for a in out]

    def grad_ref(self, g, ym=None, ys=None, dtype=np.float64):
        """``grad_scales`` is a batch sum: it is judged against ``sum_b |term_bk|``."""
        gl, gy, gs, cond = MO.log_prob_grads(self.y, self.rows, self.locs, self.scales, g, ym, ys, dtype)
        return (gl, gy, gs), (None, None, cond)

    def logits(self, rows):
        return rows


def check(what, got, ref64, ref32):
    """The base bound and the finite mask against a reference computed once."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref64)
    bound = BASE * np.maximum(1.0, np.abs(ref64))
    record_parity(what, got, ref64, ref32, err, bound)
    fin = np.isfinite(ref64)
    np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=what)
    ratio = float((err[fin] / bound[fin]).max()) if fin.any() else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the bound"


def refs(case, y, ym=None, ys=None):
    return case.ref(y, case.rows, ym, ys), case.ref(y, case.rows, ym, ys, np.float32)


def check_op(what, case, **want):
    """The case's inputs as they are through ``op``; returns the op's outputs and the fp64 reference."""
    r64, r32 = refs(case, case.y)
    out = case.op(_dev(case.y), _dev(case.rows), **want)
    check(what, out[0].cpu().numpy(), r64, r32)
    return out, r64


def forward_variants(tag, case):
    """Fast and precise math, y broadcast from one row, the rows as a column view of a wider
    NaN-filled tensor, fused y_mean / y_std and, for draws, a draw stride larger than B * row stride."""
    y, rows = case.y, case.rows
    B, W = rows.shape[-2:]
    dy, dr = _dev(y), _dev(rows)
    r64, r32 = refs(case, y)
    check(f"{tag} fast", case.op(dy, dr)[0].cpu().numpy(), r64, r32)
    prev = ops.set_math_mode("precise")
    try:
        got = case.op(dy, dr)[0].cpu().numpy()
    finally:
        ops.set_math_mode(prev)
    check(f"{tag} precise", got, r64, r32)
    check(f"{tag} y-broadcast", case.op(dy[:1], dr)[0].cpu().numpy(), *refs(case, y[:1]))
    wide = torch.full(rows.shape[:-1] + (W + 5,), float("nan"), device="cuda")
    wide[..., 3:3 + W] = dr
    view = wide[..., 3:3 + W]
    assert B == 1 or view.stride(-2) == W + 5
    check(f"{tag} column-view", case.op(dy, view)[0].cpu().numpy(), r64, r32)
    if rows.ndim == 3:
        S = rows.shape[0]
        assert S == 1 or view.stride(0) == B * (W + 5)
        tall = torch.full((S, B + 3, W), float("nan"), device="cuda")
        tall[:, :B] = dr
        part = tall[:, :B]
        assert S == 1 or part.stride(0) == (B + 3) * W
        check(f"{tag} draw-stride", case.op(dy, part)[0].cpu().numpy(), r64, r32)
    ym, ys = _norm(case.d)
    check(f"{tag} fused-norm", case.op(dy, dr, ym, ys)[0].cpu().numpy(), *refs(case, y, ym, ys))


def stress(what, case, kind):
    """A stress scaling the case was made with, or every other logit -inf; returns the fp64 reference."""
    if kind == "alternate-minus-inf":
        case.logits(case.rows)[..., ::2] = -np.inf  # every other logit removes its component
    return check_op(what, case)[1]


def nonfinite_rows(what, case, rows):
    """Exactly ``rows`` are non-finite, in the reference and on the GPU, and are counted."""
    (out, osum, nf), ref = check_op(what, case, want_nonfinite=True)
    assert list(np.flatnonzero(~np.isfinite(ref))) == rows
    assert list(np.flatnonzero(~np.isfinite(out.cpu().numpy()))) == rows
    assert float(nf.item()) == float(len(rows))
    assert not np.isfinite(osum.item())


def out_sum(case):
    args = (_dev(case.y), _dev(case.rows))
    out, s1, nf = case.op(*args, want_nonfinite=True)
    want = out.double().cpu().numpy()
    assert abs(s1.item() - float(np.sum(want))) <= 1e-12 * float(np.abs(want).sum())
    assert nf.item() == 0.0
    _, s2, _ = case.op(*args, want_nonfinite=True)
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()  # bitwise across runs
    none, s3, _ = case.op(*args, want_values=False, want_nonfinite=True)
    assert none is None
    assert s1.cpu().numpy().tobytes() == s3.cpu().numpy().tobytes()  # and without the (B,) output


def check_grads(what, case, g, ym=None, ys=None, widened=False):
    """logp at the base bound; every gradient array finite and at ``1e-5 * max(1, c)`` per element,
    c its conditioning where the case names one and ``|ref64|`` otherwise.  ``widened``:
    ``1e-5 * max(1, |ref64|) + 4 * max|ref32 - ref64|``.  Returns the GPU's arrays."""
    lp, *got = case.grad(g, ym, ys)
    r64, conds = case.grad_ref(g, ym, ys, np.float64)
    r32, _ = case.grad_ref(g, ym, ys, np.float32)
    check(what + " logp", lp, *refs(case, case.y, ym, ys))
    worst = {}
    for name, arr, ref64, ref32, cond in zip(case.grad_names, got, r64, r32, conds):
        assert np.isfinite(ref64).all()
        assert np.isfinite(arr).all(), f"{what} {name}: non-finite gradient"
        err = np.abs(arr.astype(np.float64) - ref64)
        with np.errstate(invalid="ignore"):
            dev32 = float(np.nanmax(np.abs(ref32.astype(np.float64) - ref64)))
        plain = BASE * np.maximum(1.0, np.abs(ref64))
        if widened:
            bound = plain + 4.0 * dev32
        elif cond is not None:
            bound = BASE * np.maximum(1.0, cond)
        else:
            bound = plain
        record_parity(f"{what} {name}", arr, ref64, ref32, err, bound, kind="gradient")
        worst[name] = float((err / bound).max())
        print(f"{what} {name}: max err / bound = {worst[name]:.3f} (/ plain bound = {float((err / plain).max()):.3f}); "
              f"max err = {err.max():.3e}, mirror max dev = {dev32:.3e}, "
              f"err / mirror dev = {err.max() / max(dev32, 1e-300):.3f}")
    assert all(v <= 1.0 for v in worst.values()), f"{what}: {worst}"
    return got


def gradient_walk(tag, case, g, widened=False, check=None):
    """Fast math, fused y_mean / y_std, precise math, each through ``check`` (a module's own
    wrapper of ``check_grads``; None: ``check_grads`` itself)."""
    check = check or check_grads
    check(tag, case, g, widened=widened)
    check(tag + " fused-norm", case, g, *_norm(case.d), widened=widened)
    prev = ops.set_math_mode("precise")
    try:
        check(tag + " precise", case, g, widened=widened)
    finally:
        ops.set_math_mode(prev)
