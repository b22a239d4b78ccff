"""Oracle of the mean-field draw and KL(q || p) (nfn_meanfield.hip, include/nfn.h): a torch
restatement of the formulas, in fp64 (the reference the GPU tests compare against, gradients by
autograd) and in fp32 in the same op order (the mirror whose own error the parity rule admits).

Per element, with ``m = loc``, ``s = 1e-3 + softplus(log(e - 1) + 0.05 rho)``, ``p = prior_loc``
(0 when None) and ``sp = prior_scale`` (rounded to fp32 first: the C ABI takes a float):

    w            = m + s * eps
    exact KL     = sum log(sp / s) + (s^2 + (m - p)^2) / (2 sp^2) - 1/2
    sampled KL   = sum -log s - eps^2 / 2 + log sp + (w - p)^2 / (2 sp^2)
    map mode (rho = eps = None): q = Normal(loc, 1) converted by its mean, w = m,
    exact KL     = sum log sp + (1 + (m - p)^2) / (2 sp^2) - 1/2
    sampled KL   = sum log sp + (m - p)^2 / (2 sp^2)
"""

import numpy as np
import torch

LOG_EXPM1_ONE = float(np.log(np.expm1(1.0)))


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float32)).to(dtype).reshape(-1)


def scale(rho: torch.Tensor) -> torch.Tensor:
    return 1e-3 + torch.nn.functional.softplus(LOG_EXPM1_ONE + 0.05 * rho)


def draw_kl_terms(loc, rho, eps, prior_loc=None, prior_scale=1.0, kl_exact=True):
    """``(w, per-element KL terms)`` on torch tensors of one dtype (differentiable)."""
    sp = torch.tensor(float(np.float32(prior_scale)), dtype=loc.dtype)
    p = torch.zeros_like(loc) if prior_loc is None else prior_loc
    if rho is None:  # map mode
        w = loc
        if kl_exact:
            return w, torch.log(sp) + (1.0 + (loc - p) ** 2) / (2 * sp ** 2) - 0.5
        return w, torch.log(sp) + (loc - p) ** 2 / (2 * sp ** 2)
    s = scale(rho)
    w = loc + s * eps
    if kl_exact:
        return w, torch.log(sp / s) + (s ** 2 + (loc - p) ** 2) / (2 * sp ** 2) - 0.5
    return w, -torch.log(s) - 0.5 * eps ** 2 + torch.log(sp) + (w - p) ** 2 / (2 * sp ** 2)


def draw_kl(loc, rho, eps, prior_loc=None, prior_scale=1.0, kl_exact=True, dtype=torch.float64):
    """``(w, KL)`` as numpy fp64 from fp32 inputs, evaluated in ``dtype``."""
    w, terms = draw_kl_terms(_t(loc, dtype), _t(rho, dtype), _t(eps, dtype), _t(prior_loc, dtype), prior_scale,
                             kl_exact)
    return w.double().numpy(), float(terms.double().sum())


def draw_kl_grads(loc, rho, eps, prior_loc=None, prior_scale=1.0, kl_exact=True, g_w=None, g_kl=0.0,
                  dtype=torch.float64):
    """``(grad_loc, grad_rho | None, grad_prior_loc)`` of ``sum(g_w * w) + g_kl * KL`` by
    autograd, as numpy fp64; the prior mean counts as zeros when None."""
    loc_, rho_, eps_ = _t(loc, dtype), _t(rho, dtype), _t(eps, dtype)
    prior_ = torch.zeros_like(loc_) if prior_loc is None else _t(prior_loc, dtype)
    leaves = [loc_, prior_] + ([] if rho_ is None else [rho_])
    for v in leaves:
        v.requires_grad_(True)
    w, terms = draw_kl_terms(loc_, rho_, eps_, prior_, prior_scale, kl_exact)
    # the scalar upstream gradient in the kernel's precision: a device float[1]
    loss = float(np.float32(g_kl)) * terms.sum()
    if g_w is not None:
        loss = loss + (_t(g_w, dtype) * w).sum()
    loss.backward()
    zero = torch.zeros_like(loc_)
    out = [(zero if v.grad is None else v.grad).double().numpy() for v in leaves]
    return out[0], (out[2] if rho_ is not None else None), out[1]


def make_inputs(N, seed=0, prior=False):
    """The GPU tests' inputs: ``loc ~ N(0, 1)`` with a few at +-30, ``rho`` uniform on
    [-400, 400] (``s`` from its 1e-3 floor to about 21), ``eps ~ N(0, 1)`` with 0 and +-5,
    ``g_w ~ N(0, 1)``, and a prior mean ``~ N(0, 1)`` (or None)."""
    rng = np.random.default_rng(seed)
    loc = rng.standard_normal(N).astype(np.float32)
    rho = rng.uniform(-400.0, 400.0, N).astype(np.float32)
    eps = rng.standard_normal(N).astype(np.float32)
    g_w = rng.standard_normal(N).astype(np.float32)
    for arr, vals in ((loc, (30.0, -30.0)), (eps, (0.0, 5.0, -5.0))):
        for v in vals:
            if N:
                arr[rng.integers(0, N)] = v
    p = rng.standard_normal(N).astype(np.float32) if prior else None
    return loc, rho, eps, g_w, p
