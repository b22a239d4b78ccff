"""Mean-field draw and KL, host side: the C ABI's symbols, argument validation and workspace
sizes, and the ops layer's length checks (every call here fails validation or is a host query,
so nothing reaches a GPU)."""

import os

import numpy as np
import pytest

from normalizingflownetwork_amd import _lib, ops

P = 0x1000  # never dereferenced: every call below fails validation
NAMES = ("nfn_mean_field_workspace_doubles", "nfn_mean_field_draw_kl_f32", "nfn_mean_field_draw_kl_grad_f32")


def _fwd(lib, loc=P, rho=P, eps=P, prior=None, ps=1.0, N=10, exact=1, w=P, kl=None, ws=None):
    return lib.nfn_mean_field_draw_kl_f32(loc, rho, eps, prior, ps, N, exact, w, kl, ws, None)


def _grad(lib, loc=P, rho=P, eps=P, prior=None, ps=1.0, N=10, exact=1, gw=P, gkl=P, gl=P, gr=P, gp=None):
    return lib.nfn_mean_field_draw_kl_grad_f32(loc, rho, eps, prior, ps, N, exact, gw, gkl, gl, gr, gp, None)


def _rejected(lib, rc, word):
    assert rc == _lib.NFN_E_SHAPE
    msg = lib.nfn_last_error()
    assert msg and word in msg, msg


def test_symbols_in_header_and_signatures(native_lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nfn.h")).read()
    for name in NAMES:
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert hasattr(native_lib, name)
    assert len(_lib.SIGNATURES["nfn_mean_field_draw_kl_f32"][1]) == 11
    assert len(_lib.SIGNATURES["nfn_mean_field_draw_kl_grad_f32"][1]) == 13
    assert native_lib.nfn_version() == 203


@pytest.mark.parametrize("call", [_fwd, _grad])
def test_abi_rejections_shared_by_both_entries(native_lib, call):
    _rejected(native_lib, call(native_lib, N=-1), b"batch")
    for ps in (0.0, -1.0, float("inf"), float("nan")):
        _rejected(native_lib, call(native_lib, ps=ps), b"prior_scale")
    _rejected(native_lib, call(native_lib, rho=None), b"rho and eps")
    _rejected(native_lib, call(native_lib, eps=None), b"rho and eps")


def test_abi_rejections_of_the_forward(native_lib):
    _rejected(native_lib, _fwd(native_lib, kl=P, ws=None), b"workspace")
    _rejected(native_lib, _fwd(native_lib, w=None, kl=None), b"neither")
    _rejected(native_lib, _fwd(native_lib, w=None, kl=None, ws=P), b"neither")


def test_abi_rejections_of_the_backward(native_lib):
    _rejected(native_lib, _grad(native_lib, gr=None), b"grad_rho")
    # map mode has no rho, so it needs no grad_rho: N = 0 passes validation and launches nothing
    assert _grad(native_lib, rho=None, eps=None, gr=None, N=0) == _lib.NFN_OK


def test_abi_accepts_an_empty_vector_up_to_the_launch(native_lib):
    assert _fwd(native_lib, N=0) == _lib.NFN_OK
    assert _fwd(native_lib, rho=None, eps=None, N=0) == _lib.NFN_OK
    assert _grad(native_lib, N=0, gw=None, gkl=None) == _lib.NFN_OK
    assert native_lib.nfn_last_error() == b""


def test_abi_workspace_sizes(native_lib):
    fn = native_lib.nfn_mean_field_workspace_doubles
    sizes = [fn(N) for N in (1, 3, 1024, 1025, 70001, 1 << 22, 1 << 26, 1 << 33)]
    assert all(s >= 4 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] < sizes[-1]
    assert sizes[-2] == sizes[-1]  # the grid is capped: 2^26 elements and beyond are one launch
    assert fn(0) == 0 and fn(-5) == 0


@pytest.mark.parametrize("fn", [ops.mean_field_draw_kl, ops.mean_field_draw_kl_grad, ops.mean_field_draw_kl_diff])
def test_ops_reject_mismatched_lengths(fn):
    a = lambda n: np.zeros(n, np.float32)
    with pytest.raises(AssertionError, match="rho must have 5"):
        fn(a(5), a(4), a(5))
    with pytest.raises(AssertionError, match="eps must have 5"):
        fn(a(5), a(5), a(6))
    with pytest.raises(AssertionError, match="prior_loc must have 5"):
        fn(a(5), a(5), a(5), prior_loc=a(3))
    with pytest.raises(AssertionError, match="both"):
        fn(a(5), None, a(5))
    with pytest.raises(AssertionError, match="prior_scale"):
        fn(a(5), a(5), a(5), prior_scale=0.0)


def test_ops_grad_rejects_a_mismatched_upstream_gradient():
    a = lambda n: np.zeros(n, np.float32)
    with pytest.raises(AssertionError, match="g_w must have 5"):
        ops.mean_field_draw_kl_grad(a(5), a(5), a(5), g_w=a(7))
