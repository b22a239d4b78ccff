"""The C-ABI library loads and exports every symbol include/nfn.h declares; host-side
validation (no GPU needed: every case here fails before any HIP call)."""

import ctypes
import os
import re

import pytest

from conftest import REPO
from oracle import nfn_oracle as O


def header_symbols():
    src = open(os.path.join(REPO, "include", "nfn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nfn_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_expected_entry_points():
    syms = header_symbols()
    for s in ("nfn_chain_logprob_f32", "nfn_flow_fwd_ldj_f32", "nfn_posterior_lse_f32", "nfn_version",
              "nfn_last_error", "nfn_param_size", "nfn_total_param_size", "nfn_set_math_mode"):
        assert s in syms


def test_library_exports_every_header_symbol(native_lib):
    from normalizingflownetwork_amd import _lib

    for s in header_symbols():
        assert hasattr(native_lib, s), f"{s} not exported by {_lib.LIB_NAME}"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    # and nothing the binding expects is missing from the header
    assert set(_lib.SIGNATURES) == set(header_symbols())


def test_exported_symbols_are_c_linkage(native_lib):
    from normalizingflownetwork_amd import _lib
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (nfn_[a-z0-9_]+)$", out, flags=re.M))
    assert set(header_symbols()) <= exported


def test_version(native_lib):
    # 200: out_sum is double[2] and the workspace needs no initialisation; 201: + the
    # additive nfn_split_blocks_f32; 202: + the additive nfn_flow_vjp_f32; 203: + the
    # measurement hook nfn_set_launch_events (include/nfn.h)
    from normalizingflownetwork_amd import _lib

    assert native_lib.nfn_version() == _lib.ABI_VERSION == 203
    hdr = open(os.path.join(REPO, "include", "nfn.h")).read()
    assert re.search(r"#define NFN_ABI_VERSION 203\b", hdr)


def test_launch_events_hook_arms_and_clears(native_lib):
    # host-only: arming and clearing the pending pair launches nothing (no GPU needed)
    assert native_lib.nfn_set_launch_events(None, None) == 0


def _ids(*names):
    return (ctypes.c_int32 * max(1, len(names)))(*[O.FLOW_IDS[n] for n in names])


@pytest.mark.parametrize("d", [1, 2, 3, 8, 16, 32])
def test_param_sizes_match_python(native_lib, d):
    for f in ("planar", "radial", "affine"):
        assert native_lib.nfn_param_size(O.FLOW_IDS[f], d) == O.param_size(f, d)
    ft = ("planar", "radial", "affine", "radial")
    for tr in (0, 1):
        assert native_lib.nfn_total_param_size(ctypes.cast(_ids(*ft), ctypes.c_void_p), len(ft), d, tr) == \
            O.total_param_size(ft, d, bool(tr))


def test_bad_arguments_are_rejected_before_launch(native_lib):
    lib = native_lib
    assert lib.nfn_param_size(7, 1) == -2
    assert lib.nfn_param_size(0, 0) == -1
    assert lib.nfn_param_size(0, 33) == -1
    assert b"n_dims" in lib.nfn_last_error()
    bad = (ctypes.c_int32 * 1)(5)
    assert lib.nfn_total_param_size(ctypes.cast(bad, ctypes.c_void_p), 1, 1, 0) == -2
    # too many flows
    many = (ctypes.c_int32 * 65)(*([1] * 65))
    assert lib.nfn_total_param_size(ctypes.cast(many, ctypes.c_void_p), 65, 1, 0) == -2
    ids = ctypes.cast(_ids("planar", "radial"), ctypes.c_void_p)
    fake = 0x1000  # never dereferenced: every call below fails validation first
    # negative batch
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 8, -1, 1, ids, 2, 1, None, None, fake, None, None, None) == -1
    # row stride smaller than P
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 4, 10, 1, ids, 2, 1, None, None, fake, None, None, None) == -1
    # y_mean without y_std
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 8, 10, 1, ids, 2, 1, fake, None, fake, None, None, None) == -3
    # sum requested without workspace
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 8, 10, 1, ids, 2, 1, None, None, fake, fake, None, None) == -3
    # NULL y
    assert lib.nfn_chain_logprob_f32(None, 1, fake, 8, 10, 1, ids, 2, 1, None, None, fake, None, None, None) == -3
    # a batch longer than one chunk (2^24 + 1 samples runs as two launches) is validated as a
    # whole before the first launch: no chunk may run before the call is rejected
    big = (1 << 24) + 1
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 8, big, 1, ids, 2, 1, None, None, fake, fake, None, None) == -3
    assert b"workspace" in lib.nfn_last_error()
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 8, big, 1, ids, 2, 1, fake, None, fake, None, None, None) == -3
    assert lib.nfn_chain_logprob_f32(fake, 1, fake, 4, big, 1, ids, 2, 1, None, None, fake, None, None, None) == -1
    # bad flow id in the single-flow entry point
    assert lib.nfn_flow_fwd_ldj_f32(9, fake, 1, fake, 3, 10, 1, fake, fake, None) == -2
    assert lib.nfn_flow_fwd_ldj_f32(0, fake, 1, fake, 2, 10, 1, fake, fake, None) == -1  # stride < 2d+1
    # the one-launch Chain: unknown flow id, row stride shorter than the blocks' span,
    # negative offset, NULL offsets; B = 0 is a no-op
    offs = (ctypes.c_int32 * 2)(3, 0)
    bad = (ctypes.c_int32 * 2)(0, 9)
    assert lib.nfn_chain_fwd_ldj_f32(fake, 1, fake, 6, 10, 1, bad, offs, 2, fake, fake, None) == -2
    assert lib.nfn_chain_fwd_ldj_f32(fake, 1, fake, 5, 10, 1, ids, offs, 2, fake, fake, None) == -1
    neg = (ctypes.c_int32 * 2)(3, -1)
    assert lib.nfn_chain_fwd_ldj_f32(fake, 1, fake, 6, 10, 1, ids, neg, 2, fake, fake, None) == -1
    assert lib.nfn_chain_fwd_ldj_f32(fake, 1, fake, 6, 10, 1, ids, None, 2, fake, fake, None) == -3
    assert lib.nfn_chain_fwd_ldj_f32(fake, 1, fake, 6, 0, 1, ids, offs, 2, fake, fake, None) == 0
    # posterior with zero draws
    assert lib.nfn_posterior_lse_f32(fake, 1, fake, 80, 8, 0, 10, 1, ids, 2, 1, None, None, fake, None, None,
                                     None) == -1
    assert lib.nfn_set_math_mode(3) == -1


def test_workspace_size(native_lib):
    assert native_lib.nfn_chain_workspace_doubles(0, 1, 32) == 0
    # one partial per workgroup at any tile size (>= 64 rows per tile)
    for B in (1, 1000, 1 << 22, 1 << 24):
        for d, P in ((1, 32), (8, 140)):
            assert native_lib.nfn_chain_workspace_doubles(B, d, P) >= -(-B // 64)


def test_python_binding_fails_loudly_without_device(native_lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a device is visible")
    from normalizingflownetwork_amd import ops

    with pytest.raises(RuntimeError):
        ops.chain_log_prob([[0.0]], [[0.0] * 8], ("radial", "radial"), 1, True)


def test_comm_entry_points_validate_before_rccl(native_lib):
    """nfn_comm_init / nfn_allreduce_mean reject bad arguments without touching
    RCCL or the device (multi-GPU boundary, include/nfn.h)."""
    from normalizingflownetwork_amd import _lib

    h = ctypes.c_void_p()
    uid = (ctypes.c_uint8 * _lib.NFN_COMM_ID_BYTES)()
    p_uid = ctypes.cast(uid, ctypes.c_void_p)
    assert native_lib.nfn_comm_init(ctypes.byref(h), 0, p_uid, 0) == _lib.NFN_E_SHAPE
    assert native_lib.nfn_comm_init(ctypes.byref(h), 2, p_uid, 2) == _lib.NFN_E_SHAPE
    assert native_lib.nfn_comm_init(ctypes.byref(h), 2, None, 0) == _lib.NFN_E_NULLPTR
    assert native_lib.nfn_comm_unique_id(None) == _lib.NFN_E_NULLPTR
    assert native_lib.nfn_allreduce_mean(None, None, 1, None, None, None) == _lib.NFN_E_NULLPTR
    assert "allreduce" in _lib.last_error()
    assert native_lib.nfn_comm_destroy(None) == _lib.NFN_OK


FAKE = 0x1000          # a device pointer that is never dereferenced: every row returns before a HIP call
FAKE_ODD = 0x1004      # the same, 4 bytes off a 16-byte boundary
TOO_MANY_ROWS = 1 << 40  # more tiles than a 32-bit grid holds, for every tile height


def _table(call):
    """``rejected(code, word, **kw)`` / ``accepted(**kw)`` over ``call``'s keyword overrides:
    each row changes the named arguments of one valid call."""
    from normalizingflownetwork_amd import _lib

    def rejected(code, word, **kw):
        assert call(**kw) == code, (kw, _lib.last_error())
        assert word in _lib.last_error(), (kw, _lib.last_error())

    def accepted(**kw):
        assert call(**kw) == _lib.NFN_OK, (kw, _lib.last_error())
        assert _lib.last_error() == "", kw

    return rejected, accepted


def _vp(*values):
    return ctypes.cast((ctypes.c_int32 * len(values))(*values), ctypes.c_void_p)


def _program_rows(rejected, wide):
    """The flow-program checks every chain-family entry reports first (``wide``: strides that
    are long enough for any d)."""
    from normalizingflownetwork_amd import _lib

    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0, **wide)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=33, **wide)
    rejected(_lib.NFN_E_FLOW_ID, "number of flows", ids=_vp(*([1] * 65)), K=65, **wide)
    rejected(_lib.NFN_E_FLOW_ID, "number of flows", K=-1)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 3", ids=_vp(0, 3))
    rejected(_lib.NFN_E_NULLPTR, "flow_ids", ids=None)
    # the program's errors come before the shape and the NULL-pointer errors
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 3", ids=_vp(0, 3), B=-1)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0, B=-1, **wide)


def test_grid_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    ids = _ids("planar", "radial")
    p_ids = ctypes.cast(ids, ctypes.c_void_p)
    f = native_lib.nfn_chain_logprob_grid_f32
    assert f(None, 1, 4, None, 8, 10, 1, p_ids, 2, 1, None, None, None, 10, None) == _lib.NFN_E_NULLPTR
    assert f(None, 1, -1, None, 8, 10, 1, p_ids, 2, 1, None, None, None, 10, None) == _lib.NFN_E_SHAPE
    assert f(None, 1, 4, None, 8, 10, 1, p_ids, 2, 1, None, None, None, 9, None) == _lib.NFN_E_SHAPE
    assert f(None, 1, 0, None, 8, 10, 1, p_ids, 2, 1, None, None, None, 10, None) == _lib.NFN_OK

    def call(yg=FAKE, ygs=1, G=4, t=FAKE, t_rs=8, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None, ys=None, out=FAKE, ogs=10):
        return f(yg, ygs, G, t, t_rs, B, d, ids, K, tr, ym, ys, out, ogs, None)

    rejected, accepted = _table(call)
    _program_rows(rejected, dict(ygs=64, t_rs=4096))
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "grid", G=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", ygs=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", t_rs=-8)
    rejected(_lib.NFN_E_SHAPE, "y_grid stride", d=3, ygs=2, t_rs=64)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7)
    rejected(_lib.NFN_E_SHAPE, "out grid stride", ogs=9)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ym=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ys=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y_grid", yg=None)
    rejected(_lib.NFN_E_NULLPTR, "out is NULL", out=None)
    rejected(_lib.NFN_E_NULLPTR, "t is NULL", t=None)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=TOO_MANY_ROWS, ogs=TOO_MANY_ROWS)
    # shape errors before NULL-pointer errors
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7, yg=None)
    rejected(_lib.NFN_E_SHAPE, "out grid stride", ogs=9, ym=FAKE)
    # an empty batch or grid is a no-op whatever the pointers, after the shape and pair checks
    accepted(B=0, yg=None, t=None, out=None, ogs=0)
    accepted(G=0, yg=None, t=None, out=None)
    accepted(B=0, ygs=0, t_rs=0, ids=None, K=0, tr=0)
    rejected(_lib.NFN_E_SHAPE, "t row stride", B=0, t_rs=7)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", G=0, ym=FAKE)


def test_dense_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    ids = _ids("planar", "radial")
    p_ids = ctypes.cast(ids, ctypes.c_void_p)
    f = native_lib.nfn_chain_logprob_dense_f32
    args = lambda H, hs, d=1: (None, 1, None, hs, H, None, None, 10, d, p_ids, 2, 1, None, None, None, None,  # noqa: E731
                               None, None)
    assert f(*args(16, 16)) == _lib.NFN_E_NULLPTR
    assert f(*args(10, 12)) == _lib.NFN_E_SHAPE       # H not a power of two
    assert f(*args(16, 8)) == _lib.NFN_E_SHAPE        # row stride < H
    assert f(*args(16, 18)) == _lib.NFN_E_SHAPE       # row stride not a multiple of 4
    assert "dense" in _lib.last_error() or "stride" in _lib.last_error()

    def call(y=FAKE, ybs=1, h=FAKE, hs=16, H=16, W=FAKE, bias=None, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None,
             ys=None, out=FAKE, osum=None, ws=None):
        return f(y, ybs, h, hs, H, W, bias, B, d, ids, K, tr, ym, ys, out, osum, ws, None)

    rejected, accepted = _table(call)
    _program_rows(rejected, dict(ybs=64))
    _dense_rows(rejected, accepted)
    rejected(_lib.NFN_E_NULLPTR, "workspace", osum=FAKE)
    rejected(_lib.NFN_E_SHAPE, "16-byte", h=FAKE_ODD, osum=FAKE)     # h's alignment before the workspace
    accepted(out=None)                                               # nothing requested
    accepted(B=0, y=None, h=None, W=None, out=None)
    accepted(B=0, ybs=0)
    rejected(_lib.NFN_E_SHAPE, "h row stride", B=0, hs=8)


def _dense_rows(rejected, accepted):
    """The checks the three fused-Dense entries share (one valid call: d = 1, P = 8, H = 16)."""
    from normalizingflownetwork_amd import _lib

    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "y batch stride", ybs=-1)
    rejected(_lib.NFN_E_SHAPE, "y batch stride", d=3, ybs=2)
    for H in (0, 2, 10, 128):
        rejected(_lib.NFN_E_SHAPE, "hidden width H", H=H, hs=128)
    rejected(_lib.NFN_E_SHAPE, "1 <= P <= 64", ids=None, K=0, tr=0)                 # P = 0
    rejected(_lib.NFN_E_SHAPE, "1 <= P <= 64", ids=_vp(*([0] * 21)), K=21)          # P = 65
    rejected(_lib.NFN_E_SHAPE, "n_dims <= 8", d=9, ybs=9, ids=_vp(2), K=1)          # P = 36
    rejected(_lib.NFN_E_SHAPE, "h row stride", hs=8)
    rejected(_lib.NFN_E_SHAPE, "h row stride", hs=18)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ym=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ys=FAKE)
    for name in ("y", "h", "W"):
        rejected(_lib.NFN_E_NULLPTR, "y, h or W is NULL", **{name: None})
    rejected(_lib.NFN_E_SHAPE, "16-byte", h=FAKE_ODD)
    # shape errors before NULL-pointer errors; the NULL check before h's alignment
    rejected(_lib.NFN_E_SHAPE, "hidden width H", H=10, ym=FAKE)
    rejected(_lib.NFN_E_SHAPE, "h row stride", hs=8, y=None)
    rejected(_lib.NFN_E_NULLPTR, "y, h or W is NULL", y=None, h=FAKE_ODD)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", B=0, ym=FAKE)


def test_posterior_dense_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_posterior_lse_dense_f32
    p_ids = _vp(0, 1)  # planar, radial at d = 1: P = 8

    def call(y=FAKE, ybs=1, h=FAKE, hds=160, hs=16, H=16, W=FAKE, wds=128, bias=FAKE, bds=8, S=3, B=10, d=1, ids=p_ids,
             K=2, tr=1, ym=None, ys=None, out=FAKE, osum=None, ws=None):
        return f(y, ybs, h, hds, hs, H, W, wds, bias, bds, S, B, d, ids, K, tr, ym, ys, out, osum, ws, None)

    rejected, accepted = _table(call)
    _program_rows(rejected, dict(ybs=64))
    _dense_rows(rejected, accepted)
    rejected(_lib.NFN_E_SHAPE, "draws", S=0)
    for hds in (-4, 162, 156):                                       # negative, no multiple of 4, < B * h_rowstride
        rejected(_lib.NFN_E_SHAPE, "h draw stride", hds=hds)
    rejected(_lib.NFN_E_SHAPE, "W draw stride", wds=-1)
    rejected(_lib.NFN_E_SHAPE, "W draw stride", wds=127)
    rejected(_lib.NFN_E_SHAPE, "bias draw stride", bds=-1)
    rejected(_lib.NFN_E_SHAPE, "bias draw stride", bds=7)
    rejected(_lib.NFN_E_NULLPTR, "workspace", osum=FAKE)
    rejected(_lib.NFN_E_SHAPE, "16-byte", h=FAKE_ODD, osum=FAKE)
    rejected(_lib.NFN_E_SHAPE, "draws", S=0, ym=FAKE)
    accepted(out=None)
    accepted(B=0, y=None, h=None, W=None, bias=None, out=None, hds=0)
    accepted(B=0, S=1, wds=0, bds=0, hds=0)                          # one draw: the draw strides are unused
    rejected(_lib.NFN_E_SHAPE, "h row stride", B=0, hs=8, hds=0)


def test_dense_grad_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_chain_logprob_dense_grad_f32
    p_ids = _vp(0, 1)

    def call(y=FAKE, ybs=1, h=FAKE, hs=16, H=16, W=FAKE, bias=None, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None, ys=None,
             g=None, lp=FAKE, gh=FAKE, ghs=16, gW=FAKE, gb=FAKE, gy=FAKE, ws=FAKE):
        return f(y, ybs, h, hs, H, W, bias, B, d, ids, K, tr, ym, ys, g, lp, gh, ghs, gW, gb, gy, ws, None)

    rejected, accepted = _table(call)
    _program_rows(rejected, dict(ybs=64))
    _dense_rows(rejected, accepted)
    rejected(_lib.NFN_E_SHAPE, "grad_h row stride", ghs=15)
    rejected(_lib.NFN_E_NULLPTR, "workspace", ws=None)
    rejected(_lib.NFN_E_NULLPTR, "workspace", ws=None, gW=None)
    rejected(_lib.NFN_E_SHAPE, "16-byte", h=FAKE_ODD, ws=None)
    rejected(_lib.NFN_E_SHAPE, "exceed LDS", H=64, hs=64, ghs=64, ids=_vp(*([2] * 31)), K=31)   # P = 64, K d = 31
    accepted(B=0, y=None, h=None, W=None, gW=None, gb=None, ws=None)
    rejected(_lib.NFN_E_SHAPE, "grad_h row stride", B=0, ghs=15)


def test_split_blocks_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_split_blocks_f32
    w3 = (ctypes.c_int32 * 3)(3, 3, 2)
    p_w = ctypes.cast(w3, ctypes.c_void_p)
    assert f(None, 8, 10, p_w, 3, None, None) == _lib.NFN_E_NULLPTR      # t / dst NULL
    assert f(None, 8, 10, None, 3, None, None) == _lib.NFN_E_NULLPTR     # widths NULL
    assert f(None, 8, 10, p_w, 0, None, None) == _lib.NFN_E_SHAPE        # no blocks
    assert f(None, 7, 10, p_w, 3, None, None) == _lib.NFN_E_SHAPE        # row stride < 8
    assert "stride" in _lib.last_error()
    w0 = (ctypes.c_int32 * 2)(3, 0)
    assert f(None, 8, 10, ctypes.cast(w0, ctypes.c_void_p), 2, None, None) == _lib.NFN_E_SHAPE
    assert f(None, 8, 0, p_w, 3, None, None) == _lib.NFN_OK              # empty batch: nothing to do

    def call(t=FAKE, t_rs=8, B=10, w=p_w, n=3, dst=FAKE):
        return f(t, t_rs, B, w, n, dst, None)

    rejected, accepted = _table(call)
    rejected(_lib.NFN_E_SHAPE, "nblocks", n=0)
    rejected(_lib.NFN_E_SHAPE, "nblocks", n=65)
    rejected(_lib.NFN_E_NULLPTR, "widths", w=None)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", t_rs=-1)
    rejected(_lib.NFN_E_SHAPE, "block widths", w=_vp(3, 0), n=2)
    rejected(_lib.NFN_E_SHAPE, "1024", w=_vp(1000, 25), n=2, t_rs=1025)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7)
    rejected(_lib.NFN_E_NULLPTR, "t or dst", t=None)
    rejected(_lib.NFN_E_NULLPTR, "t or dst", dst=None)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=1 << 31)
    # the block count before the widths pointer, the widths pointer before the batch
    rejected(_lib.NFN_E_SHAPE, "nblocks", n=0, w=None)
    rejected(_lib.NFN_E_NULLPTR, "widths", w=None, B=-1)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7, t=None)
    accepted(B=0, t=None, dst=None)
    rejected(_lib.NFN_E_SHAPE, "stride", B=0, t_rs=-1)


def test_flow_vjp_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_flow_vjp_f32
    fake = 0x1000  # never dereferenced
    assert f(9, fake, 1, fake, 3, 10, 1, None, None, fake, fake, None) == _lib.NFN_E_FLOW_ID
    assert f(0, fake, 1, fake, 2, 10, 1, None, None, fake, fake, None) == _lib.NFN_E_SHAPE    # stride < 2d+1
    assert f(1, fake, 1, fake, 3, 10, 0, None, None, fake, fake, None) == _lib.NFN_E_SHAPE    # n_dims 0
    assert f(1, fake, 1, fake, 3, -1, 1, None, None, fake, fake, None) == _lib.NFN_E_SHAPE    # negative batch
    assert f(1, None, 1, fake, 3, 10, 1, None, None, fake, fake, None) == _lib.NFN_E_NULLPTR  # NULL z
    assert "NULL" in _lib.last_error()
    assert f(1, fake, 1, fake, 3, 10, 1, None, None, None, None, None) == _lib.NFN_OK         # nothing requested
    assert f(1, fake, 1, fake, 3, 0, 1, None, None, fake, fake, None) == _lib.NFN_OK          # empty batch
    _flow_rows(lambda id=1, z=FAKE, zbs=1, tk=FAKE, t_rs=3, B=10, d=1, o1=FAKE, o2=FAKE:
               f(id, z, zbs, tk, t_rs, B, d, None, None, o1, o2, None))


def _flow_rows(call):
    """The validation nfn_flow_fwd_ldj_f32 and nfn_flow_vjp_f32 share (``o1``, ``o2``: the two
    outputs; the valid call is a radial flow at d = 1)."""
    from normalizingflownetwork_amd import _lib

    rejected, accepted = _table(call)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=33, zbs=33, t_rs=128)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 9", id=9)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id -1", id=-1)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", zbs=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", t_rs=-3)
    rejected(_lib.NFN_E_SHAPE, "z batch stride", d=3, zbs=2, t_rs=8)
    rejected(_lib.NFN_E_SHAPE, "t row stride", id=0, t_rs=2)          # planar: 2 d + 1 = 3
    rejected(_lib.NFN_E_SHAPE, "t row stride", id=2, d=4, zbs=4, t_rs=7)
    rejected(_lib.NFN_E_NULLPTR, "z or t_k is NULL", z=None)
    rejected(_lib.NFN_E_NULLPTR, "z or t_k is NULL", tk=None)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=TOO_MANY_ROWS)
    # n_dims before the flow id, the flow id before the shape, the shape before the pointers
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0, id=9)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 9", id=9, B=-1)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=2, z=None)
    accepted(o1=None, o2=None, z=None, tk=None)                        # nothing requested
    accepted(B=0, z=None, tk=None)
    accepted(B=0, zbs=0, t_rs=0)
    rejected(_lib.NFN_E_SHAPE, "t row stride", B=0, t_rs=2)


def test_flow_fwd_ldj_entry_point_validates(native_lib):
    f = native_lib.nfn_flow_fwd_ldj_f32
    _flow_rows(lambda id=1, z=FAKE, zbs=1, tk=FAKE, t_rs=3, B=10, d=1, o1=FAKE, o2=FAKE:
               f(id, z, zbs, tk, t_rs, B, d, o1, o2, None))


def test_sample_entry_point_validates(native_lib):
    """nfn_chain_sample_f32 returns the documented codes and sets nfn_last_error before any
    HIP call (no pointer below is dereferenced)."""
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_chain_sample_f32
    fake = 0x1000
    p_ids = ctypes.cast(_ids("planar", "radial"), ctypes.c_void_p)  # d = 1: P = 3 + 3 + 2 = 8

    def call(eps_bs=1, t_rs=8, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None, ys=None, eps=fake, t=fake, y=fake, lp=fake):
        return f(eps, eps_bs, t, t_rs, B, d, ids, K, tr, ym, ys, y, lp, None)

    def rejected(code, word, **kw):
        assert call(**kw) == code, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())

    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0, t_rs=64)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=33, t_rs=4096)
    many = (ctypes.c_int32 * 65)(*([1] * 65))
    rejected(_lib.NFN_E_FLOW_ID, "number of flows", ids=ctypes.cast(many, ctypes.c_void_p), K=65, t_rs=4096)
    bad = (ctypes.c_int32 * 2)(0, 3)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 3", ids=ctypes.cast(bad, ctypes.c_void_p))
    rejected(_lib.NFN_E_NULLPTR, "flow_ids", ids=None)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "eps", d=3, eps_bs=2, t_rs=64)   # eps_bstride in (0, d)
    rejected(_lib.NFN_E_SHAPE, "eps", eps_bs=-1)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7)           # t_rowstride in (0, P)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=-8)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ym=fake)               # y_mean without y_std
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ys=fake)
    rejected(_lib.NFN_E_NULLPTR, "eps", eps=None)
    rejected(_lib.NFN_E_NULLPTR, "y_out", y=None)
    rejected(_lib.NFN_E_NULLPTR, "t is NULL", t=None)
    # an empty batch is a no-op whatever the pointers; broadcast strides (0) are legal
    assert call(B=0, eps=None, t=None, y=None, lp=None) == _lib.NFN_OK
    assert call(B=0, eps=None, t=None, y=None, lp=None, eps_bs=0, t_rs=0) == _lib.NFN_OK
    assert call(B=0, eps=None, t=None, y=None, lp=None, ids=None, K=0, tr=0, t_rs=0) == _lib.NFN_OK
    assert _lib.last_error() == ""
    # the bad shape is reported before the empty batch returns
    assert call(B=0, t_rs=7) == _lib.NFN_E_SHAPE
    rejected(_lib.NFN_E_NULLPTR, "y_mean", B=0, ym=fake)
    rejected(_lib.NFN_E_FLOW_ID, "number of flows", K=-1)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=TOO_MANY_ROWS)
    # the program's errors before the shape errors, the shape errors before the NULL pointers
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 3", ids=ctypes.cast(bad, ctypes.c_void_p), B=-1)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0, B=-1, t_rs=64)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7, eps=None)
    rejected(_lib.NFN_E_SHAPE, "eps", eps_bs=-1, ym=fake)


def _chain_rows(rejected, accepted):
    """The checks the forward, posterior and backward chain entries share (the valid call:
    planar + radial at d = 1 with a trainable base, P = 8)."""
    from normalizingflownetwork_amd import _lib

    _program_rows(rejected, dict(ybs=64, t_rs=4096))
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", ybs=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", t_rs=-8)
    rejected(_lib.NFN_E_SHAPE, "y batch stride", d=3, ybs=2, t_rs=64)
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ym=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ys=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y is NULL", y=None)
    rejected(_lib.NFN_E_NULLPTR, "t is NULL", t=None)
    # shape errors before NULL-pointer errors
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=7, y=None)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1, ym=FAKE)
    # an empty batch is a no-op whatever the pointers, after the shape and pair checks
    accepted(B=0, y=None, t=None, out=None)
    accepted(B=0, ybs=0, t_rs=0, ids=None, K=0, tr=0)
    rejected(_lib.NFN_E_SHAPE, "t row stride", B=0, t_rs=7)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", B=0, ym=FAKE)


def test_forward_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_chain_logprob_f32
    p_ids = _vp(0, 1)

    def call(y=FAKE, ybs=1, t=FAKE, t_rs=8, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None, ys=None, out=FAKE, osum=None,
             ws=None):
        return f(y, ybs, t, t_rs, B, d, ids, K, tr, ym, ys, out, osum, ws, None)

    rejected, accepted = _table(call)
    _chain_rows(rejected, accepted)
    rejected(_lib.NFN_E_NULLPTR, "workspace", osum=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y is NULL", y=None, osum=FAKE)
    accepted(out=None)                                                  # nothing requested
    accepted(out=None, t=None, t_rs=0, ids=None, K=0, tr=0)
    # a batch longer than one chunk is checked as a whole before its first launch
    big = (1 << 24) + 1
    rejected(_lib.NFN_E_SHAPE, "batch", B=-big)
    rejected(_lib.NFN_E_SHAPE, "t row stride", B=big, t_rs=7)
    rejected(_lib.NFN_E_SHAPE, "y batch stride", B=big, d=3, ybs=2, t_rs=64)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", B=big, ys=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y is NULL", B=big, y=None)
    rejected(_lib.NFN_E_NULLPTR, "t is NULL", B=big, t=None)
    rejected(_lib.NFN_E_NULLPTR, "workspace", B=big, osum=FAKE)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 3", B=big, ids=_vp(0, 3), osum=FAKE)
    accepted(B=big, out=None)


def test_posterior_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_posterior_lse_f32
    p_ids = _vp(0, 1)

    def call(y=FAKE, ybs=1, t=FAKE, t_ds=80, t_rs=8, S=4, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None, ys=None, out=FAKE,
             osum=None, ws=None):
        return f(y, ybs, t, t_ds, t_rs, S, B, d, ids, K, tr, ym, ys, out, osum, ws, None)

    rejected, accepted = _table(call)
    _chain_rows(rejected, accepted)
    rejected(_lib.NFN_E_SHAPE, "draws", S=0)
    rejected(_lib.NFN_E_SHAPE, "draws", S=-2)
    rejected(_lib.NFN_E_SHAPE, "stride", t_ds=-80)
    rejected(_lib.NFN_E_NULLPTR, "workspace", osum=FAKE)
    rejected(_lib.NFN_E_SHAPE, "draws", S=0, ym=FAKE)
    rejected(_lib.NFN_E_SHAPE, "draws", S=0, B=0)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=TOO_MANY_ROWS)     # the posterior is never chunked
    accepted(out=None)
    accepted(B=0, t_ds=0, S=1)


def test_grad_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_chain_logprob_grad_f32
    p_ids = _vp(0, 1)

    def call(y=FAKE, ybs=1, t=FAKE, t_rs=8, B=10, d=1, ids=p_ids, K=2, tr=1, ym=None, ys=None, g=None, out=FAKE,
             gt=FAKE, gt_rs=8, gy=FAKE):
        return f(y, ybs, t, t_rs, B, d, ids, K, tr, ym, ys, g, out, gt, gt_rs, gy, None)

    rejected, accepted = _table(call)
    _chain_rows(rejected, accepted)
    rejected(_lib.NFN_E_SHAPE, "grad_t row stride", gt_rs=7)
    rejected(_lib.NFN_E_SHAPE, "grad_t row stride", gt_rs=-8)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=TOO_MANY_ROWS)
    rejected(_lib.NFN_E_SHAPE, "grad_t row stride", gt_rs=7, ym=FAKE)
    accepted(out=None, gt=None, gy=None, y=None, t=None)                # nothing requested
    accepted(out=None, gt=None, gy=None, gt_rs=0)                       # no grad_t: its stride is not read
    rejected(_lib.NFN_E_SHAPE, "grad_t row stride", B=0, gt_rs=7)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", out=None, gt=None, gy=None, ys=FAKE)


def _mixture_rows(rejected, accepted, rs_word):
    """The checks every entry of the two mixture families makes (``rs``: the row stride of the
    logits / parameter rows).  Unlike the chain family they check the pointers before an empty
    batch returns."""
    from normalizingflownetwork_amd import _lib

    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=33, ybs=33, rs=1 << 20)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "y batch stride", ybs=-1)
    rejected(_lib.NFN_E_SHAPE, "y batch stride", d=3, ybs=2, rs=1 << 10)
    rejected(_lib.NFN_E_SHAPE, rs_word, rs=4)
    rejected(_lib.NFN_E_SHAPE, rs_word, rs=-100)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ym=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "y_mean", ys=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "is NULL", y=None)
    rejected(_lib.NFN_E_NULLPTR, "is NULL", t=None)
    rejected(_lib.NFN_E_SHAPE, rs_word, rs=4, y=None)                 # shape before pointers
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1, ym=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "is NULL", B=0, y=None)               # pointers before the empty batch
    rejected(_lib.NFN_E_NULLPTR, "y_mean", B=0, ym=FAKE)
    rejected(_lib.NFN_E_SHAPE, rs_word, B=0, rs=4)
    accepted(B=0)
    accepted(B=0, ybs=0)


def _sum_rows(rejected):
    from normalizingflownetwork_amd import _lib

    rejected(_lib.NFN_E_NULLPTR, "workspace", osum=FAKE)
    rejected(_lib.NFN_E_NULLPTR, "workspace", osum=FAKE, B=0)
    rejected(_lib.NFN_E_NULLPTR, "is NULL", y=None, osum=FAKE)


def _draw_rows(rejected, accepted):
    from normalizingflownetwork_amd import _lib

    rejected(_lib.NFN_E_SHAPE, "draws", S=0)
    rejected(_lib.NFN_E_SHAPE, "draws", S=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", ds=-1)
    rejected(_lib.NFN_E_SHAPE, "draws", S=0, y=None)
    accepted(B=0, ds=0)


def test_kernel_mixture_entry_points_validate(native_lib):
    from normalizingflownetwork_amd import _lib

    lib = native_lib

    def fwd(y=FAKE, ybs=1, t=FAKE, rs=100, locs=FAKE, scales=FAKE, B=10, d=1, M=100, ym=None, ys=None, out=FAKE,
            osum=None, ws=None):
        return lib.nfn_kernel_mixture_logprob_f32(y, ybs, t, rs, locs, scales, B, d, M, ym, ys, out, osum, ws, None)

    def grad(y=FAKE, ybs=1, t=FAKE, rs=100, locs=FAKE, scales=FAKE, B=10, d=1, M=100, ym=None, ys=None, g=None,
             out=FAKE, gl=FAKE, glrs=100, gy=FAKE, gs=None, ws=None):
        return lib.nfn_kernel_mixture_logprob_grad_f32(y, ybs, t, rs, locs, scales, B, d, M, ym, ys, g, out, gl, glrs,
                                                       gy, gs, ws, None)

    def post(y=FAKE, ybs=1, t=FAKE, ds=1000, rs=100, S=4, locs=FAKE, scales=FAKE, B=10, d=1, M=100, ym=None, ys=None,
             out=FAKE, osum=None, ws=None):
        return lib.nfn_posterior_lse_kernel_mixture_f32(y, ybs, t, ds, rs, S, locs, scales, B, d, M, ym, ys, out, osum,
                                                        ws, None)

    for call in (fwd, grad, post):
        rejected, accepted = _table(call)
        _mixture_rows(rejected, accepted, "logits row stride")
        rejected(_lib.NFN_E_SHAPE, "number of kernels M", M=0)
        rejected(_lib.NFN_E_SHAPE, "number of kernels M", M=1025, rs=1025)
        rejected(_lib.NFN_E_SHAPE, "M * n_dims", M=1024, d=32, ybs=32, rs=1024)
        rejected(_lib.NFN_E_SHAPE, "number of kernels M", M=0, d=0)      # M before n_dims
        rejected(_lib.NFN_E_NULLPTR, "is NULL", locs=None)
        rejected(_lib.NFN_E_NULLPTR, "is NULL", scales=None)
        if call is not grad:
            _sum_rows(rejected)
    rejected, accepted = _table(grad)
    rejected(_lib.NFN_E_SHAPE, "grad_logits row stride", glrs=99)
    rejected(_lib.NFN_E_NULLPTR, "workspace", gs=FAKE)                 # grad_scales needs its workspace
    rejected(_lib.NFN_E_NULLPTR, "workspace", gs=FAKE, B=0)
    rejected(_lib.NFN_E_NULLPTR, "is NULL", y=None, gs=FAKE)
    rejected(_lib.NFN_E_SHAPE, "grad_logits row stride", glrs=99, gs=FAKE)
    accepted(B=0, gl=None, glrs=0)
    _draw_rows(*_table(post))


def test_gaussian_mixture_entry_points_validate(native_lib):
    from normalizingflownetwork_amd import _lib

    lib = native_lib

    def fwd(y=FAKE, ybs=1, t=FAKE, rs=15, B=10, d=1, K=5, ym=None, ys=None, out=FAKE, osum=None, ws=None):
        return lib.nfn_gaussian_mixture_logprob_f32(y, ybs, t, rs, B, d, K, ym, ys, out, osum, ws, None)

    def grad(y=FAKE, ybs=1, t=FAKE, rs=15, B=10, d=1, K=5, ym=None, ys=None, g=None, out=FAKE, gt=FAKE, gtrs=15,
             gy=FAKE):
        return lib.nfn_gaussian_mixture_logprob_grad_f32(y, ybs, t, rs, B, d, K, ym, ys, g, out, gt, gtrs, gy, None)

    def post(y=FAKE, ybs=1, t=FAKE, ds=150, rs=15, S=4, B=10, d=1, K=5, ym=None, ys=None, out=FAKE, osum=None,
             ws=None):
        return lib.nfn_posterior_lse_gaussian_mixture_f32(y, ybs, t, ds, rs, S, B, d, K, ym, ys, out, osum, ws, None)

    for call in (fwd, grad, post):
        rejected, accepted = _table(call)
        _mixture_rows(rejected, accepted, "t row stride")
        rejected(_lib.NFN_E_SHAPE, "number of components K", K=0)
        rejected(_lib.NFN_E_SHAPE, "row width", K=342, rs=1026)           # P = 1026 > 1023
        rejected(_lib.NFN_E_SHAPE, "row width", K=1 << 30, d=32, ybs=32, rs=1 << 40)
        rejected(_lib.NFN_E_SHAPE, "number of components K", K=0, d=0)   # K before n_dims
        if call is not grad:
            _sum_rows(rejected)
    rejected, accepted = _table(grad)
    rejected(_lib.NFN_E_SHAPE, "grad_t row stride", gtrs=14)
    rejected(_lib.NFN_E_SHAPE, "grad_t row stride", gtrs=14, y=None)
    accepted(B=0, gt=None, gtrs=0)
    _draw_rows(*_table(post))


def test_chain_fwd_ldj_entry_point_validates(native_lib):
    from normalizingflownetwork_amd import _lib

    f = native_lib.nfn_chain_fwd_ldj_f32
    p_ids, offs = _vp(0, 1), _vp(3, 0)   # planar then radial at d = 1, the layer's reversed blocks

    def call(z=FAKE, zbs=1, t=FAKE, t_rs=6, B=10, d=1, ids=p_ids, offs=offs, K=2, zo=FAKE, lo=FAKE):
        return f(z, zbs, t, t_rs, B, d, ids, offs, K, zo, lo, None)

    rejected, accepted = _table(call)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0)
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=33, zbs=33)
    rejected(_lib.NFN_E_FLOW_ID, "number of flows", K=65)
    rejected(_lib.NFN_E_FLOW_ID, "number of flows", K=-1)
    rejected(_lib.NFN_E_NULLPTR, "flow_ids or block_offsets", ids=None)
    rejected(_lib.NFN_E_NULLPTR, "flow_ids or block_offsets", offs=None)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", zbs=-1)
    rejected(_lib.NFN_E_SHAPE, "stride", t_rs=-6)
    rejected(_lib.NFN_E_SHAPE, "z batch stride", d=3, zbs=2, t_rs=64)
    rejected(_lib.NFN_E_FLOW_ID, "unknown flow id 9", ids=_vp(0, 9))
    rejected(_lib.NFN_E_SHAPE, "negative block offset", offs=_vp(3, -1))
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=5)
    rejected(_lib.NFN_E_NULLPTR, "z or t is NULL", z=None)
    rejected(_lib.NFN_E_NULLPTR, "z or t is NULL", t=None)
    rejected(_lib.NFN_E_SHAPE, "batch too large", B=TOO_MANY_ROWS, offs=_vp(0, 3))   # not the layer's layout
    # n_dims before the flow count, the two arrays before the batch, the batch before the flow ids
    rejected(_lib.NFN_E_SHAPE, "n_dims", d=0, K=65)
    rejected(_lib.NFN_E_NULLPTR, "flow_ids or block_offsets", ids=None, B=-1)
    rejected(_lib.NFN_E_SHAPE, "batch", B=-1, ids=_vp(0, 9))
    rejected(_lib.NFN_E_SHAPE, "t row stride", t_rs=5, z=None)
    accepted(zo=None, lo=None, z=None, t=None)                          # nothing requested
    accepted(B=0, z=None, t=None)
    accepted(B=0, zbs=0, t_rs=0, ids=None, offs=None, K=0)
    rejected(_lib.NFN_E_SHAPE, "t row stride", B=0, t_rs=5)
