"""Device-side entry points: torch device tensors in, HIP kernels via the C ABI.

Every function here launches a kernel from ``libnfn_hip.so`` on torch's
current HIP stream; torch provides only device memory and the stream handle.
There is no CPU fallback — without a GPU these raise ``RuntimeError``.
"""

from __future__ import annotations

import collections
import contextlib
import ctypes
import threading
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

FLOW_IDS = {"planar": 0, "radial": 1, "affine": 2}

def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("normalizingflownetwork_amd needs a HIP device (MI355X); none is visible")
    return torch.device("cuda", torch.cuda.current_device())


def as_device_f32(x, device: Optional[torch.device] = None) -> torch.Tensor:
    """Convert array-likes / tensors to a float32 device tensor whose last dim is contiguous."""
    dev = device or _device()
    if isinstance(x, torch.Tensor):
        t = x.to(device=dev, dtype=torch.float32)
    else:
        t = torch.as_tensor(np.asarray(x, dtype=np.float32), device=dev)
    if t.dim() >= 1 and t.shape[-1] > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t


def _row_stride(x: torch.Tensor) -> int:
    """Batch stride in elements of a (N, W) tensor; 0 broadcasts a single row."""
    return 0 if x.shape[0] == 1 else int(x.stride(0))


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _ptr(x: Optional[torch.Tensor]) -> Optional[int]:
    return None if x is None else int(x.data_ptr())


def flow_ids(flow_types: Sequence[str]):
    for f in flow_types:
        assert f in FLOW_IDS, f"unknown flow type {f!r}"  # DistributionLayers.py:231
    ids = (ctypes.c_int32 * max(1, len(flow_types)))(*[FLOW_IDS[f] for f in flow_types])
    return ids, len(flow_types)


def param_size(flow_type: str, n_dims: int) -> int:
    """Host metadata, same as the C ABI's ``nfn_param_size``: ``PlanarFlow.py:35-41`` (2d+1),
    ``RadialFlow.py:36-42`` (d+2), ``AffineFlow.py:11-17`` (2d)."""
    assert flow_type in FLOW_IDS, f"unknown flow type {flow_type!r}"
    return {"planar": 2 * n_dims + 1, "radial": n_dims + 2, "affine": 2 * n_dims}[flow_type]


def total_param_size(flow_types: Sequence[str], n_dims: int, trainable_base: bool) -> int:
    """``InverseNormalizingFlowLayer.get_total_param_size`` (``DistributionLayers.py:257-265``)."""
    return sum(param_size(f, n_dims) for f in flow_types) + (2 * n_dims if trainable_base else 0)


def flow_block_offsets(flow_types: Sequence[str], n_dims: int, trainable_base: bool) -> list:
    """Column of each row of ``t`` where flow k's block starts, in the layer's reversed layout
    (``_get_bijector``, ``DistributionLayers.py:267-278``): the base's ``2 n_dims`` columns when
    trainable, then the blocks of the LAST flow type first."""
    off, offs = 2 * int(n_dims) if trainable_base else 0, [0] * len(flow_types)
    for k in reversed(range(len(flow_types))):
        offs[k] = off
        off += param_size(flow_types[k], n_dims)
    return offs


_workspaces: "collections.OrderedDict" = collections.OrderedDict()
_ws_lock = threading.Lock()
# (device, stream) workspaces kept at once; the least recently used is dropped beyond
# this (pooled / side streams come and go: fit's capture stream, the bench's ring).
WORKSPACE_CACHE_ENTRIES = 8
# Workspaces a captured HIP graph may hold the address of: handed out while their stream
# was capturing, as (pin sequence number, (device, stream) key, workspace).  A graph's replays
# write partials and the ticket there, so the block must not go back to the allocator while
# the graph lives.  Graphs do not tell when they die: an entry stays pinned for the life of
# the process unless the capturing code takes it over and keeps it next to its graph.
# ``capture_graph`` does that: use it to capture.  Its two primitives (``graph_pin_mark`` before
# a capture, ``take_graph_workspaces`` after it) are scoped by the mark, not only by the stream,
# because stream handles are pooled and reused: pins made before the mark (another live
# graph's) stay where they are.
_graph_workspaces: list = []
_pin_seq = 0


def graph_pin_mark() -> int:
    """The pin sequence number before a capture: ``take_graph_workspaces(stream, mark)`` then
    hands back exactly the workspaces that capture pinned."""
    with _ws_lock:
        return _pin_seq


def take_graph_workspaces(stream, since: int) -> list:
    """Unpin and return the workspaces pinned on ``stream`` (a torch stream) since ``since``
    (a ``graph_pin_mark()``): the caller keeps them alive exactly as long as the graph
    captured there.  Pins made before the mark, on this stream handle or any other, stay."""
    key = (stream.device.index, int(stream.cuda_stream))
    with _ws_lock:
        return _take_pins(key, since)


def _take_pins(key, since: int) -> list:
    mine = [ws for seq, k, ws in _graph_workspaces if k == key and seq >= since]
    _graph_workspaces[:] = [(seq, k, ws) for seq, k, ws in _graph_workspaces if not (k == key and seq >= since)]
    return mine


@contextlib.contextmanager
def side_stream(device, stream=None):
    """Run the body on a side stream (``stream``, or a new one) that first waits on the current one, which
    waits on it afterwards: a step is warmed up and captured off the default stream (capture rules)."""
    side = torch.cuda.Stream(device=device) if stream is None else stream
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        yield side
    torch.cuda.current_stream(device).wait_stream(side)


class CapturedGraph:
    """A captured HIP ``graph``, its ``replay()``, and the ``workspaces`` its capture pinned, which
    live exactly as long as this object."""

    def __init__(self, graph, workspaces: list):
        self.graph, self.workspaces, self.replay = graph, workspaces, graph.replay


def capture_graph(fn, device, stream=None) -> CapturedGraph:
    """Capture the launches of ``fn()`` on a side stream (``stream``, to share the one a warm-up
    ran on, or a new one) into a HIP graph, taking over the workspaces the capture pinned.  The
    capture executes nothing; warming ``fn`` up beforehand is the caller's business."""
    graph = torch.cuda.CUDAGraph()
    with side_stream(device, stream) as side:
        mark = graph_pin_mark()
        with torch.cuda.graph(graph, stream=side):
            fn()
    return CapturedGraph(graph, take_graph_workspaces(side, mark))


def _pin(key, ws) -> None:
    """Pin ``ws`` for a capture on ``key`` (caller holds ``_ws_lock``).  A block already pinned
    by an earlier capture that nobody took stays pinned for the process: not pinned again."""
    global _pin_seq
    if not any(p is ws for _, _, p in _graph_workspaces):
        _graph_workspaces.append((_pin_seq, key, ws))
        _pin_seq += 1


def _workspace(n_doubles: int, device: torch.device) -> torch.Tensor:
    """The workspace of the current (device, stream): calls are ordered on their stream,
    so calls in flight on different streams never share partials, the posterior's split
    region or the finishing ticket.  No initialisation is needed (ABI 200: the ticket
    carries a per-call epoch).  Dropping (or outgrowing) an entry that no graph captured
    is safe: its memory returns to the caching allocator's pool of the SAME stream, so a
    later allocation that reuses it is ordered after the calls that used it.  An entry
    used during a capture is pinned instead (``_graph_workspaces``): the graph keeps its
    address, and eager warm-up calls on the capture stream commonly allocate it first."""
    stream = torch.cuda.current_stream(device)
    key = (device.index, int(stream.cuda_stream))
    capturing = torch.cuda.is_current_stream_capturing()
    with _ws_lock:
        ws = _workspaces.get(key)
        if ws is None or ws.numel() < n_doubles:
            ws = torch.empty(max(2, n_doubles), dtype=torch.float64, device=device)
        if capturing:
            _pin(key, ws)
        _workspaces[key] = ws
        _workspaces.move_to_end(key)
        while len(_workspaces) > WORKSPACE_CACHE_ENTRIES:
            _workspaces.popitem(last=False)
        return ws


def _with_nonfinite(out, osum, want_nonfinite: bool):
    """``(out, sum)`` or, with ``want_nonfinite``, ``(out, sum, nonfinite)``: ``osum`` is the
    kernel's (2,) fp64 {sum, non-finite count}; ``nonfinite`` counts the inf / NaN values
    among the summed log-densities (next to the partial sums in the kernel; SURVEY.md §5,
    the reference's ``TerminateOnNaN``, ``BaseEstimator.py:29``)."""
    s = None if osum is None else osum[0:1]
    if not want_nonfinite:
        return out, s
    return out, s, osum[1:2]


def _prep_2d(x, width: int, name: str, device) -> torch.Tensor:
    x = as_device_f32(x, device)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    assert x.dim() == 2, f"{name} must be 2-D (batch, {width}), got shape {tuple(x.shape)}"
    assert x.shape[-1] == width, f"{name} last dimension must be {width}, got {x.shape[-1]}"
    return x


def _norm_stats(y_mean, y_std, n_dims: int, device):
    """``y_mean`` / ``y_std`` as (n_dims,) device arrays, or ``(None, None)``.  The kernels
    read ``n_dims`` floats of each, so every entry point checks the lengths here."""
    if y_mean is None:
        return None, None
    ym = as_device_f32(y_mean, device).reshape(-1).contiguous()
    ys = as_device_f32(y_std, device).reshape(-1).contiguous()
    assert ym.numel() == n_dims and ys.numel() == n_dims, f"y_mean and y_std must have {n_dims} elements"
    return ym, ys


def _upstream(g_out, B: int, device) -> Optional[torch.Tensor]:
    """The upstream gradient ``g_out`` as a (B,) device array (None => ones in the kernel)."""
    if g_out is None:
        return None
    g = as_device_f32(g_out, device).reshape(-1).contiguous()
    assert g.numel() == B, f"g_out must have {B} elements"
    return g


def _param_rows(t, P: int, device):
    """``(t, row stride, rows)`` of the chain's parameter rows ``t`` (B or 1, P); an empty
    chain over a fixed base (P = 0) reads nothing and gets one dummy row."""
    if P == 0:
        return torch.zeros((1, 1), dtype=torch.float32, device=device), 0, 1
    t = _prep_2d(t, P, "t", device)
    return t, _row_stride(t), int(t.shape[0])


def _chain_inputs(y, t, flow_types: Sequence[str], n_dims: int, trainable_base: bool, device, name: str = "y"):
    """``(y, t, t_stride, B, P)`` of a chain entry: ``y`` (B or 1, d) against ``t`` (B or 1, P)."""
    P = total_param_size(flow_types, n_dims, trainable_base)
    y = _prep_2d(y, n_dims, name, device)
    t, t_stride, rows = _param_rows(t, P, device)
    B = max(int(y.shape[0]), rows)
    assert y.shape[0] in (1, B) and rows in (1, B), "incompatible batch sizes"
    return y, t, t_stride, B, P


def _row_inputs(y, rows, width: int, n_dims: int, y_mean, y_std, device, name: str):
    """``(y, rows, row stride, y_mean, y_std, B)`` of a mixture entry: ``rows`` (B, width) with a
    unit column stride (a column view of a wider tensor stays a view), ``y`` (B or 1, d).  The
    ABI's rows have a stride >= width, so a single row against a batch of ``y`` and an expanded
    (stride-0) batch are materialised."""
    y = _prep_2d(y, n_dims, "y", device)
    rows = _prep_2d(rows, width, name, device)
    B = max(int(y.shape[0]), int(rows.shape[0]))
    assert y.shape[0] in (1, B) and rows.shape[0] in (1, B), "incompatible batch sizes"
    if rows.shape[0] != B:
        rows = rows.expand(B, width).contiguous()
    stride = int(rows.stride(0)) if B > 1 else width
    if stride < width:
        rows, stride = rows.contiguous(), width
    return (y, rows, stride) + _norm_stats(y_mean, y_std, n_dims, device) + (B,)


def _sum_outputs(B: int, want_values: bool, want_sum: bool, workspace_doubles, device, workspace: bool = False):
    """``(out (B,) | None, out_sum (2,) fp64 | None, workspace | None)`` of a summing entry.
    ``workspace_doubles()`` sizes the stream's workspace, taken with ``want_sum`` (or always,
    with ``workspace``)."""
    out = torch.empty((B,), dtype=torch.float32, device=device) if want_values else None
    osum = torch.empty((2,), dtype=torch.float64, device=device) if want_sum else None
    ws = _workspace(int(workspace_doubles()), device) if (want_sum or workspace) else None
    return out, osum, ws


def _unbroadcast(grad: Optional[torch.Tensor], x: torch.Tensor, B: int) -> Optional[torch.Tensor]:
    """The per-sample gradient rows summed for an input that was one row broadcast over B."""
    if grad is not None and x.shape[0] == 1 and B > 1:
        return grad.sum(0, keepdim=True)
    return grad


def chain_log_prob(
    y,
    t,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
    want_values: bool = True,
    want_sum: bool = False,
    want_nonfinite: bool = False,
):
    """Fused ``log_prob(y | t)`` over the whole flow chain (one kernel launch).

    Returns ``(log_prob (B,) float32 | None, sum (1,) float64 | None)``, plus the
    non-finite count (1,) fp64 when ``want_nonfinite`` (implies ``want_sum``).
    With ``y_mean``/``y_std`` it is ``BaseEstimator.log_pdf``'s
    ``log_prob((y-mu)/sigma) - sum(log sigma)`` (``BaseEstimator.py:77-86``).
    """
    dev = _device()
    y, t, t_stride, B, P = _chain_inputs(y, t, flow_types, n_dims, trainable_base, dev)
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite,
                                 lambda: lib.nfn_chain_workspace_doubles(B, n_dims, P), dev)
    ids, k = flow_ids(flow_types)
    rc = lib.nfn_chain_logprob_f32(
        _ptr(y), _row_stride(y), _ptr(t), t_stride, B, int(n_dims),
        ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys),
        _ptr(out), _ptr(osum), _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_chain_logprob_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def chain_log_prob_grad(
    y,
    t,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
    g_out=None,
    want_logp: bool = False,
    want_grad_t: bool = True,
    want_grad_y: bool = True,
):
    """Fused backward (one kernel): per sample ``dL/dt`` (B, P) and ``dL/dy`` (B, d) for
    ``L = sum_b g_out[b] * log_prob_b`` (``g_out`` None => ones), optionally ``log_prob``.

    What Keras autodiff computes through the reference's log_prob when it trains
    (``BaseEstimator.py:19-31, 55-59``).  A broadcast input (batch 1) still gets
    one gradient row per sample.  Returns ``(log_prob | None, grad_t | None, grad_y | None)``."""
    dev = _device()
    y, t, t_stride, B, P = _chain_inputs(y, t, flow_types, n_dims, trainable_base, dev)
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    g = _upstream(g_out, B, dev)
    lp = torch.empty((B,), dtype=torch.float32, device=dev) if want_logp else None
    gt = torch.empty((B, P), dtype=torch.float32, device=dev) if (want_grad_t and P > 0) else None
    gy = torch.empty((B, n_dims), dtype=torch.float32, device=dev) if want_grad_y else None
    ids, k = flow_ids(flow_types)
    rc = _lib.load().nfn_chain_logprob_grad_f32(
        _ptr(y), _row_stride(y), _ptr(t), t_stride, B, int(n_dims),
        ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys), _ptr(g),
        _ptr(lp), _ptr(gt), P if gt is not None else 0, _ptr(gy), _stream(),
    )
    _lib.check(rc, "nfn_chain_logprob_grad_f32")
    if want_grad_t and gt is None:
        gt = torch.empty((B, 0), dtype=torch.float32, device=dev)
    return lp, gt, gy


class _ChainLogProb(torch.autograd.Function):
    """``log_prob`` as a differentiable op: forward = the fused forward kernel,
    backward = the fused backward kernel (the chain is recomputed there, nothing
    but the inputs is saved)."""

    @staticmethod
    def forward(ctx, y, t, flow_types, n_dims, trainable_base, y_mean, y_std):
        out, _ = chain_log_prob(y, t, flow_types, n_dims, trainable_base, y_mean, y_std)
        ctx.save_for_backward(y, t)
        ctx.meta = (tuple(flow_types), int(n_dims), bool(trainable_base), y_mean, y_std)
        return out

    @staticmethod
    def backward(ctx, g):
        y, t = ctx.saved_tensors
        flow_types, n_dims, trainable_base, y_mean, y_std = ctx.meta
        need_y, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        _, gt, gy = chain_log_prob_grad(y, t, flow_types, n_dims, trainable_base, y_mean, y_std,
                                        g_out=g.contiguous(), want_grad_t=need_t, want_grad_y=need_y)
        B = g.shape[0]
        return _unbroadcast(gy, y, B), _unbroadcast(gt, t, B), None, None, None, None, None


def log_prob(y, t, flow_types: Sequence[str], n_dims: int, trainable_base: bool, y_mean=None, y_std=None):
    """Differentiable fused ``log_prob`` (B,): gradients w.r.t. ``t`` and ``y`` flow
    through ``torch.autograd`` via the fused backward kernel."""
    dev = _device()
    y, t, _, _, _ = _chain_inputs(y, t, flow_types, n_dims, trainable_base, dev)
    y_mean, y_std = _norm_stats(y_mean, y_std, n_dims, dev)
    return _ChainLogProb.apply(y, t, tuple(flow_types), int(n_dims), bool(trainable_base), y_mean, y_std)


class _DenseLogProb(torch.autograd.Function):
    """``log_prob(y | t = h W + b)`` as a differentiable op with the output Dense layer
    fused both ways: forward = ``nfn_chain_logprob_dense_f32``, backward =
    ``nfn_chain_logprob_dense_grad_f32`` (t is never materialised)."""

    @staticmethod
    def forward(ctx, y, h, W, b, flow_types, n_dims, trainable_base):
        out, _ = chain_log_prob_dense(y, h, W, b, flow_types, n_dims, trainable_base)
        ctx.save_for_backward(y, h, W, b)
        ctx.meta = (tuple(flow_types), int(n_dims), bool(trainable_base))
        return out

    @staticmethod
    def backward(ctx, g):
        y, h, W, b = ctx.saved_tensors
        flow_types, n_dims, trainable_base = ctx.meta
        _, gh, gW, gb, gy = chain_log_prob_dense_grad(y, h, W, b, flow_types, n_dims, trainable_base,
                                                      g_out=g.contiguous())
        return _unbroadcast(gy, y, gh.shape[0]), gh, gW, gb, None, None, None


def log_prob_dense(y, h, W, b, flow_types: Sequence[str], n_dims: int, trainable_base: bool):
    """Differentiable ``log_prob(y | h W + b)`` (B,) through the fused Dense layer: the
    gradients w.r.t. ``h``, ``W``, ``b`` (and ``y``) come from the fused backward kernel."""
    dev = _device()
    y = _prep_2d(y, n_dims, "y", dev)
    h = as_device_f32(h, dev).contiguous()
    return _DenseLogProb.apply(y, h, as_device_f32(W, dev), as_device_f32(b, dev), tuple(flow_types), int(n_dims),
                               bool(trainable_base))


DENSE_HIDDEN_WIDTHS = (4, 8, 16, 32, 64)


def dense_fusable(H: int, P: int, n_dims: int) -> bool:
    """Shapes the fused Dense->chain kernel takes (include/nfn.h, nfn_chain_logprob_dense_f32)."""
    return H in DENSE_HIDDEN_WIDTHS and 1 <= P <= 64 and n_dims <= 8


def _dense_inputs(h, W, b, P: int, n_dims: int, device):
    """``(h, W, b, B, H, fused)`` of the output Dense layer ``h`` (B, H), ``W`` (H, P), ``b`` (P,)
    or None; ``fused`` says whether the fused kernels take the shape and ``h``'s alignment."""
    h = as_device_f32(h, device)
    assert h.dim() == 2, "h must be (B, H)"
    B, H = int(h.shape[0]), int(h.shape[1])
    W = as_device_f32(W, device).contiguous()
    assert tuple(W.shape) == (H, P), f"W must be ({H}, {P})"
    bb = None if b is None else as_device_f32(b, device).reshape(-1).contiguous()
    fused = dense_fusable(H, P, n_dims) and h.stride(0) % 4 == 0 and h.data_ptr() % 16 == 0
    return h, W, bb, B, H, fused


def chain_log_prob_dense(
    y,
    h,
    W,
    b,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
    want_values: bool = True,
    want_sum: bool = False,
    want_nonfinite: bool = False,
):
    """``log_prob(y | t = h W + b)`` with the estimator's output Dense layer
    (``MaximumLikelihoodNNEstimator.py:37-44``) fused into the chain kernel: ``h`` (B, H) last
    hidden activations, ``W`` (H, P), ``b`` (P,).  Shapes the fused kernel does not take run
    as a library GEMM (torch) followed by the chain kernel."""
    dev = _device()
    P = total_param_size(flow_types, n_dims, trainable_base)
    h, W, bb, B, H, fused = _dense_inputs(h, W, b, P, n_dims, dev)
    if not fused:
        t = h @ W + (bb if bb is not None else 0.0)
        return chain_log_prob(y, t, flow_types, n_dims, trainable_base, y_mean, y_std, want_values, want_sum,
                              want_nonfinite)
    y = _prep_2d(y, n_dims, "y", dev)
    assert y.shape[0] in (1, B), "incompatible batch sizes"
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite,
                                 lambda: lib.nfn_chain_workspace_doubles(B, n_dims, P), dev)
    ids, k = flow_ids(flow_types)
    rc = lib.nfn_chain_logprob_dense_f32(
        _ptr(y), _row_stride(y), _ptr(h), int(h.stride(0)), H, _ptr(W), _ptr(bb), B, int(n_dims),
        ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys), _ptr(out), _ptr(osum),
        _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_chain_logprob_dense_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def chain_log_prob_dense_grad(
    y,
    h,
    W,
    b,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
    g_out=None,
    want_logp: bool = False,
):
    """Backward of :func:`chain_log_prob_dense` (one fused kernel + a fixed-order reduction):
    for ``L = sum_b g_out[b] * log_prob_b`` returns ``(log_prob | None, dL/dh (B, H),
    dL/dW (H, P), dL/db (P,), dL/dy (B, d))`` — what Keras autodiff takes through the output
    ``Dense(P)`` and the layer's ``log_prob`` when the reference trains
    (``MaximumLikelihoodNNEstimator.py:37-44``, ``BaseEstimator.py:19-31``), with ``t`` never
    materialised.  Shapes the fused kernel does not take run as library GEMMs around
    :func:`chain_log_prob_grad`."""
    dev = _device()
    P = total_param_size(flow_types, n_dims, trainable_base)
    h, W, bb, B, H, fused = _dense_inputs(h, W, b, P, n_dims, dev)
    y = _prep_2d(y, n_dims, "y", dev)
    assert y.shape[0] in (1, B), "incompatible batch sizes"
    g = _upstream(g_out, B, dev)
    lib = _lib.load()
    if fused:
        ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
        lp = torch.empty((B,), dtype=torch.float32, device=dev) if want_logp else None
        gh = torch.empty((B, H), dtype=torch.float32, device=dev)
        gW = torch.empty((H, P), dtype=torch.float32, device=dev)
        gb = torch.empty((P,), dtype=torch.float32, device=dev)
        gy = torch.empty((B, n_dims), dtype=torch.float32, device=dev)
        ws = torch.empty((max(1, int(lib.nfn_dense_grad_workspace_floats(B, H, P))),), dtype=torch.float32,
                         device=dev)
        ids, k = flow_ids(flow_types)
        rc = lib.nfn_chain_logprob_dense_grad_f32(
            _ptr(y), _row_stride(y), _ptr(h), int(h.stride(0)), H, _ptr(W), _ptr(bb), B, int(n_dims),
            ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys), _ptr(g), _ptr(lp),
            _ptr(gh), H, _ptr(gW), _ptr(gb), _ptr(gy), _ptr(ws), _stream(),
        )
        if rc == 0:
            return lp, gh, gW, gb, gy
        if rc != _lib.NFN_E_SHAPE:
            _lib.check(rc, "nfn_chain_logprob_dense_grad_f32")
    # unfused: t by the library GEMM, the chain backward kernel, library GEMMs for dh / dW / db
    t = h @ W + (bb if bb is not None else 0.0)
    lp, gt, gy = chain_log_prob_grad(y, t, flow_types, n_dims, trainable_base, y_mean, y_std, g, want_logp)
    return lp, gt @ W.t(), h.t() @ gt, gt.sum(0), gy


def posterior_lse_dense(
    y,
    h,
    W,
    b,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
    want_values: bool = True,
    want_sum: bool = False,
    want_nonfinite: bool = False,
):
    """Bayesian posterior score per sample with the output DenseVariational layer fused
    (``BayesianNNEstimator.py:65-76`` score over draws, ``:136-145`` the variational output
    layer): ``logsumexp_s log_prob(y | h_s W_s + b_s) - log S``.  ``h``: (S, B, H) per-draw
    last hidden activations, or (B, H) shared by every draw; ``W``: (S, H, P); ``b``: (S, P)
    or None.  Shapes the fused kernel does not take run as a library GEMM (torch) followed
    by :func:`posterior_lse`."""
    dev = _device()
    P = total_param_size(flow_types, n_dims, trainable_base)
    h = as_device_f32(h, dev)
    W = as_device_f32(W, dev).contiguous()
    assert W.dim() == 3 and W.shape[2] == P, f"W must be (S, H, {P})"
    S, H = int(W.shape[0]), int(W.shape[1])
    assert h.dim() in (2, 3) and h.shape[-1] == H, f"h must be (S, B, {H}) or (B, {H})"
    if h.dim() == 3:
        assert h.shape[0] == S, "h and W disagree on the number of draws"
    bb = None
    if b is not None:
        bb = as_device_f32(b, dev).reshape(S, P).contiguous()
    B = int(h.shape[-2])
    hrow = int(h.stride(-2))
    hdraw = int(h.stride(0)) if h.dim() == 3 else 0
    aligned = h.stride(-1) == 1 and hrow % 4 == 0 and hdraw % 4 == 0 and h.data_ptr() % 16 == 0
    if h.dim() == 3 and S > 1 and hdraw < B * hrow:
        aligned = False
    if not dense_fusable(H, P, n_dims) or not aligned:
        hd = h if h.dim() == 3 else h.unsqueeze(0).expand(S, B, H)
        t = torch.matmul(hd, W) + (bb.unsqueeze(1) if bb is not None else 0.0)
        return posterior_lse(y, t, flow_types, n_dims, trainable_base, y_mean, y_std, want_values, want_sum,
                             want_nonfinite)
    y = _prep_2d(y, n_dims, "y", dev)
    assert y.shape[0] in (1, B), "incompatible batch sizes"
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite,
                                 lambda: lib.nfn_chain_workspace_doubles(B, n_dims, P), dev)
    ids, k = flow_ids(flow_types)
    rc = lib.nfn_posterior_lse_dense_f32(
        _ptr(y), _row_stride(y), _ptr(h), hdraw, hrow, H, _ptr(W), H * P, _ptr(bb), P, S, B, int(n_dims),
        ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys), _ptr(out), _ptr(osum),
        _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_posterior_lse_dense_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def chain_sample(eps, t, flow_types: Sequence[str], n_dims: int, trainable_base: bool, y_mean=None, y_std=None,
                 want_log_prob: bool = True):
    """Draw ``y ~ p(y | t)`` through the inverted flows for given standard-normal ``eps``
    (B or 1, d): returns ``(y (B, d), log_prob (B,) | None)`` (``nfn_chain_sample_f32``).
    A capability the reference lacks (its flows define no inverse)."""
    dev = _device()
    e, t, t_stride, B, _ = _chain_inputs(eps, t, flow_types, n_dims, trainable_base, dev, name="eps")
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    y = torch.empty((B, n_dims), dtype=torch.float32, device=dev)
    lp = torch.empty((B,), dtype=torch.float32, device=dev) if want_log_prob else None
    ids, k = flow_ids(flow_types)
    rc = _lib.load().nfn_chain_sample_f32(
        _ptr(e), _row_stride(e), _ptr(t), t_stride, B, int(n_dims),
        ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys), _ptr(y), _ptr(lp),
        _stream(),
    )
    _lib.check(rc, "nfn_chain_sample_f32")
    return y, lp


def chain_log_prob_grid(
    y_grid,
    t,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
) -> torch.Tensor:
    """``log_prob`` of every grid value ``y_grid[g]`` (G, d) under every parameter row
    ``t[b]`` (B, P): returns (G, B) — the density-grid evaluation of
    ``flow_plotting.plot_model`` (``evaluation/visualization/flow_plotting.py:33-53``) in
    one kernel."""
    dev = _device()
    P = total_param_size(flow_types, n_dims, trainable_base)
    yg = _prep_2d(y_grid, n_dims, "y_grid", dev)
    t, t_stride, B = _param_rows(t, P, dev)
    G = int(yg.shape[0])
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    out = torch.empty((G, B), dtype=torch.float32, device=dev)
    ids, k = flow_ids(flow_types)
    rc = _lib.load().nfn_chain_logprob_grid_f32(
        _ptr(yg), int(yg.stride(0)) if G > 1 else 0, G, _ptr(t), t_stride, B, int(n_dims),
        ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys), _ptr(out), B,
        _stream(),
    )
    _lib.check(rc, "nfn_chain_logprob_grid_f32")
    return out


def _flow_inputs(flow_type: str, z, t_k, n_dims: int, device):
    """``(z, t_k, B, param size)`` of a single-flow entry: ``z`` (B or 1, d), ``t_k`` (B or 1, p)."""
    ps = param_size(flow_type, n_dims)
    z = _prep_2d(z, n_dims, "z", device)
    t_k = as_device_f32(t_k, device)
    if t_k.dim() == 1:
        t_k = t_k.unsqueeze(0)
    assert t_k.shape[-1] == ps, f"{flow_type} flow needs {ps} params, got {t_k.shape[-1]}"
    B = max(z.shape[0], t_k.shape[0])
    assert z.shape[0] in (1, B) and t_k.shape[0] in (1, B), "incompatible batch sizes"
    return z, t_k, B, ps


def flow_forward_ldj(flow_type: str, z, t_k, n_dims: int, want_z: bool = True, want_ldj: bool = True):
    """One bijector: ``(forward(z), forward_log_det_jacobian(z))`` (either may be None)."""
    dev = _device()
    z, t_k, B, ps = _flow_inputs(flow_type, z, t_k, n_dims, dev)
    z_out = torch.empty((B, n_dims), dtype=torch.float32, device=dev) if want_z else None
    ldj = torch.empty((B,), dtype=torch.float32, device=dev) if want_ldj else None
    lib = _lib.load()
    rc = lib.nfn_flow_fwd_ldj_f32(
        FLOW_IDS[flow_type], _ptr(z), _row_stride(z), _ptr(t_k), _row_stride(t_k), B, int(n_dims),
        _ptr(z_out), _ptr(ldj), _stream(),
    )
    _lib.check(rc, "nfn_flow_fwd_ldj_f32")
    return z_out, ldj


def flow_vjp(flow_type: str, z: torch.Tensor, t_k: torch.Tensor, n_dims: int, g_z=None, g_ldj=None,
             want_dz: bool = True, want_dt: bool = True):
    """One bijector's vector-Jacobian product (``nfn_flow_vjp_f32``): ``(dL/dz, dL/dt_k)``
    per sample, (B, d) and (B, p), for ``L = sum_b <g_z[b], f(z_b)> + g_ldj[b] fldj(z_b)``
    (``g_z`` / ``g_ldj`` None => zero).  ``z`` / ``t_k`` as ``flow_forward_ldj`` takes them."""
    dev = _device()
    z, t_k, B, ps = _flow_inputs(flow_type, z, t_k, n_dims, dev)
    gz = gl = None
    if g_z is not None:
        gz = as_device_f32(g_z, dev).expand(B, n_dims).contiguous()
    if g_ldj is not None:
        gl = as_device_f32(g_ldj, dev).reshape(-1).expand(B).contiguous()
    dz = torch.empty((B, n_dims), dtype=torch.float32, device=dev) if want_dz else None
    dt = torch.empty((B, ps), dtype=torch.float32, device=dev) if want_dt else None
    rc = _lib.load().nfn_flow_vjp_f32(
        FLOW_IDS[flow_type], _ptr(z), _row_stride(z), _ptr(t_k), _row_stride(t_k), B, int(n_dims), _ptr(gz), _ptr(gl),
        _ptr(dz), _ptr(dt), _stream(),
    )
    _lib.check(rc, "nfn_flow_vjp_f32")
    return dz, dt


class _FlowForwardLdj(torch.autograd.Function):
    """One bijector's ``(forward(z), forward_log_det_jacobian(z))`` as a differentiable op:
    forward = ``nfn_flow_fwd_ldj_f32``, backward = ``nfn_flow_vjp_f32`` (the flow is
    recomputed there from the saved inputs).  What TF's tape differentiates through
    ``PlanarFlow._forward`` / ``_forward_log_det_jacobian`` (``PlanarFlow.py:68-80``),
    ``RadialFlow.py:50-70`` and tfp ``Affine``."""

    @staticmethod
    def forward(ctx, z, t_k, flow_type, n_dims):
        ctx.set_materialize_grads(False)
        z_out, ldj = flow_forward_ldj(flow_type, z, t_k, n_dims)
        ctx.save_for_backward(z, t_k)
        ctx.meta = (flow_type, int(n_dims))
        return z_out, ldj

    @staticmethod
    def backward(ctx, g_z, g_ldj):
        z, t_k = ctx.saved_tensors
        flow_type, n_dims = ctx.meta
        need_z, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_z is None and g_ldj is None) or not (need_z or need_t):
            return None, None, None, None
        dz, dt = flow_vjp(flow_type, z, t_k, n_dims, g_z, g_ldj, want_dz=need_z, want_dt=need_t)
        B = max(z.shape[0], t_k.shape[0])
        return _unbroadcast(dz, z, B), _unbroadcast(dt, t_k, B), None, None


def flow_forward_ldj_diff(flow_type: str, z, t_k, n_dims: int):
    """Differentiable ``(forward(z), forward_log_det_jacobian(z))`` of one bijector: gradients
    w.r.t. ``z`` and ``t_k`` flow through ``torch.autograd`` via ``nfn_flow_vjp_f32``."""
    dev = _device()
    z, t_k, _, _ = _flow_inputs(flow_type, z, t_k, n_dims, dev)
    return _FlowForwardLdj.apply(z, t_k, flow_type, int(n_dims))


def split_pays(widths: Sequence[int], row_stride: int) -> bool:
    """Whether the flows' single launches should read one-pass contiguous copies of their
    blocks (``split_blocks``) rather than their strided views, by expected HBM bytes per
    sample: a view launch fetches the whole 128-B lines its block touches (about
    ``128 + 4 (w - 1)`` bytes for a block of w floats at a random offset), the split reads the
    row once and writes and re-reads the blocks (``4 row_stride + 8 sum(w)``).  The split must
    win by 30 % to pay for its own pass: C2's 3-float blocks of 32-float rows (368 vs 1360 B)
    take it, C3's 10-17-float blocks of 140-float rows (1552 vs 1612 B) do not (measured:
    1.43 vs 4.32 ms and 2.60 vs 2.02 ms, profiles/r03/r03s2_*, r03c3g_*; C3 reading the
    rows is 1.82 ms since, r03j_*)."""
    strided = sum(128 + 4 * (int(w) - 1) for w in widths)
    split = 4 * int(row_stride) + 8 * sum(int(w) for w in widths)
    return split < 0.7 * strided


def split_blocks(t: torch.Tensor, widths: Sequence[int]):
    """``[t[:, o_k:o_k + w_k].contiguous() for each block]`` in ONE pass over ``t``
    (``nfn_split_blocks_f32``): ``t`` (B, >= sum(widths)) device rows with unit column
    stride, the blocks consecutive from column 0.  The blocks are views of one allocation.
    What the TF slices of ``_get_bijector`` are (``DistributionLayers.py:267-278``: copies)."""
    assert isinstance(t, torch.Tensor) and t.dim() == 2 and t.stride(1) == 1, "t must be (B, W), unit column stride"
    widths = [int(w) for w in widths]
    B, W = int(t.shape[0]), sum(widths)
    assert t.shape[1] >= W, "t narrower than its blocks"
    buf = torch.empty((B * W,), dtype=torch.float32, device=t.device)
    arr = (ctypes.c_int32 * max(1, len(widths)))(*widths)
    rc = _lib.load().nfn_split_blocks_f32(_ptr(t), _row_stride(t), B, arr, len(widths), _ptr(buf), _stream())
    _lib.check(rc, "nfn_split_blocks_f32")
    out, off = [], 0
    for w in widths:
        out.append(buf[off:off + B * w].view(B, w))
        off += B * w
    return out


def chain_forward_ldj(flow_types: Sequence[str], z, t, block_offsets: Sequence[int], n_dims: int,
                      want_z: bool = True, want_ldj: bool = True):
    """A Chain of flows as ONE kernel launch (``nfn_chain_fwd_ldj_f32``): ``(z_K, sum_k
    log|det J_k|)`` for flows applied in ``flow_types`` order, flow k reading its block at
    column ``block_offsets[k]`` of each row of ``t`` (B or 1, >= span).  What tfp's
    ``Chain.forward`` / ``forward_log_det_jacobian`` compute over the layer's flows
    (``DistributionLayers.py:267-278``)."""
    dev = _device()
    z = _prep_2d(z, n_dims, "z", dev)
    t = as_device_f32(t, dev)
    if t.dim() == 1:
        t = t.unsqueeze(0)
    assert t.dim() == 2 and t.stride(1) == 1, "t must be (B, W) with unit column stride"
    ids, K = flow_ids(flow_types)
    assert len(block_offsets) == K, "one block offset per flow"
    offs = (ctypes.c_int32 * max(1, K))(*[int(o) for o in block_offsets])
    B = max(z.shape[0], t.shape[0])
    assert z.shape[0] in (1, B) and t.shape[0] in (1, B), "incompatible batch sizes"
    z_out = torch.empty((B, n_dims), dtype=torch.float32, device=dev) if want_z else None
    ldj = torch.empty((B,), dtype=torch.float32, device=dev) if want_ldj else None
    lib = _lib.load()
    rc = lib.nfn_chain_fwd_ldj_f32(_ptr(z), _row_stride(z), _ptr(t), _row_stride(t), B, int(n_dims), ids, offs, K,
                                   _ptr(z_out), _ptr(ldj), _stream())
    _lib.check(rc, "nfn_chain_fwd_ldj_f32")
    return z_out, ldj


def posterior_lse(
    y,
    t_draws,
    flow_types: Sequence[str],
    n_dims: int,
    trainable_base: bool,
    y_mean=None,
    y_std=None,
    want_values: bool = True,
    want_sum: bool = False,
    want_nonfinite: bool = False,
):
    """``logsumexp_s(log_pdf(y_b | t[s, b])) - log S`` per sample (``BayesianNNEstimator.py:65-76``).

    ``t_draws``: (S, B, P) device tensor (rows contiguous)."""
    dev = _device()
    P = total_param_size(flow_types, n_dims, trainable_base)
    y = _prep_2d(y, n_dims, "y", dev)
    t_draws = as_device_f32(t_draws, dev)
    assert t_draws.dim() == 3 and t_draws.shape[-1] == P, f"t_draws must be (S, B, {P})"
    S, Bt = int(t_draws.shape[0]), int(t_draws.shape[1])
    B = max(y.shape[0], Bt)
    assert y.shape[0] in (1, B) and Bt in (1, B)
    ym, ys = _norm_stats(y_mean, y_std, n_dims, dev)
    lib = _lib.load()
    # the workspace is always taken: it also enables the draw split (more parallelism for small B)
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite,
                                 lambda: lib.nfn_posterior_workspace_doubles(B, n_dims, P), dev, workspace=True)
    ids, k = flow_ids(flow_types)
    rc = lib.nfn_posterior_lse_f32(
        _ptr(y), _row_stride(y), _ptr(t_draws), int(t_draws.stride(0)), 0 if Bt == 1 else int(t_draws.stride(1)),
        S, B, int(n_dims), ctypes.cast(ids, ctypes.c_void_p), k, int(bool(trainable_base)), _ptr(ym), _ptr(ys),
        _ptr(out), _ptr(osum), _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_posterior_lse_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def set_math_mode(mode: str) -> str:
    """Select the kernels' transcendental implementation for later launches:
    ``"fast"`` (default) or ``"precise"``.  Returns the previous mode."""
    assert mode in ("fast", "precise")
    prev = _lib.load().nfn_set_math_mode(1 if mode == "precise" else 0)
    _lib.check(prev if prev < 0 else 0, "nfn_set_math_mode")
    return "precise" if prev == 1 else "fast"


# ---------------------------------------------------------------------------
# Pre-bound launchers (the benchmark / serving loop)
# ---------------------------------------------------------------------------

class _Launcher:
    """C-ABI calls bound once over fixed device buffers: all validation and pointer marshalling
    happens in the constructor, ``launch()`` makes the bound calls in order on one stream (one
    call for every launcher but ``FlowsLauncher``)."""

    def __init__(self):
        self.lib = _lib.load()
        self._calls = []  # (bound C function, its arguments but the stream, its name)

    def _bind(self, entry: str, *args) -> None:
        self._calls.append((getattr(self.lib, entry), args, entry))

    def launch(self, stream: Optional[int] = None) -> None:
        st = stream if stream is not None else _stream()
        for fn, args, entry in self._calls:
            rc = fn(*args, st)
            if rc != 0:
                _lib.check(rc, entry)

    @staticmethod
    def _check_rows(y: torch.Tensor, n_dims: int, t: torch.Tensor, P: int) -> int:
        """``y`` (B or 1, d) and ``t`` (B or 1, P) with unit column strides: returns B."""
        assert y.dim() == 2 and y.shape[1] == n_dims and y.stride(1) == 1
        assert t.dim() == 2 and t.shape[1] == P and t.stride(1) == 1
        return max(int(y.shape[0]), int(t.shape[0]))


class _SumLauncher(_Launcher):
    """A launcher of an entry that ends in ``(out, out_sum, workspace, stream)``: ``launch()``
    writes ``out`` (B,) and ``sum2`` = {fp64 sum, non-finite count}, finished in the kernel by
    its last workgroup (``sum`` is ``sum2[0:1]``); ``partials`` is the launcher's own workspace."""

    def _bind_sums(self, entry: str, *head, n_partials: int, write_values: bool, fused_sum: bool = True) -> None:
        dev = self.y.device
        self.out = torch.empty((self.B,), dtype=torch.float32, device=dev) if write_values else None
        self.sum2 = torch.zeros((2,), dtype=torch.float64, device=dev)  # {sum, non-finite}
        self.sum = self.sum2[0:1]
        self.n_partials = int(n_partials)
        self.partials = torch.zeros((max(2, self.n_partials),), dtype=torch.float64, device=dev)
        self._sum_at = len(head) + 1  # where out_sum stands among the arguments (bind_sum)
        self._bind(entry, *head, _ptr(self.out), _ptr(self.sum2) if fused_sum else None, _ptr(self.partials))

    def finish_sum(self, stream: Optional[int] = None) -> torch.Tensor:
        """The launch's fp64 sum (finished inside the kernel: nothing to launch)."""
        return self.sum

    @property
    def nonfinite(self) -> torch.Tensor:
        """(1,) fp64: non-finite values among the last launch's log-densities."""
        return self.sum2[1:2]


class DenseLauncher(_SumLauncher):
    """Pre-bound fused Dense->chain launch over fixed device buffers (benchmark loop)."""

    _entry = "nfn_chain_logprob_dense_f32"

    def __init__(self, y: torch.Tensor, h: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
                 flow_types: Sequence[str], n_dims: int, trainable_base: bool, write_values: bool = True):
        super().__init__()
        self.n_dims = int(n_dims)
        self.P = total_param_size(flow_types, n_dims, trainable_base)
        self.B, self.H = int(h.shape[-2]), int(h.shape[-1])
        assert dense_fusable(self.H, self.P, self.n_dims)
        self.y, self.h, self.W, self.b = y, h, W.contiguous(), b
        layer = self._layer_args()
        self._ids, k = flow_ids(flow_types)
        self._bind_sums(self._entry, _ptr(y), _row_stride(y), *layer, self.B, self.n_dims,
                        ctypes.cast(self._ids, ctypes.c_void_p), k, int(bool(trainable_base)), None, None,
                        n_partials=self.lib.nfn_chain_workspace_doubles(self.B, self.n_dims, self.P),
                        write_values=write_values)

    def _layer_args(self) -> tuple:
        """The entry's arguments for ``h``, ``W`` and ``b`` (checked here)."""
        assert self.h.stride(1) == 1 and tuple(self.W.shape) == (self.H, self.P)
        return _ptr(self.h), int(self.h.stride(0)), self.H, _ptr(self.W), _ptr(self.b)


class PosteriorDenseLauncher(DenseLauncher):
    """Pre-bound fused DenseVariational->posterior launch (``nfn_posterior_lse_dense_f32``):
    ``h`` (S, B, H), ``W`` (S, H, P), ``b`` (S, P) or None."""

    _entry = "nfn_posterior_lse_dense_f32"

    def _layer_args(self) -> tuple:
        h = self.h
        self.S = int(h.shape[0])
        assert h.dim() == 3 and h.is_contiguous() and tuple(self.W.shape) == (self.S, self.H, self.P)
        assert self.b is None or tuple(self.b.shape) == (self.S, self.P)
        self.b = None if self.b is None else self.b.contiguous()
        return (_ptr(h), int(h.stride(0)), int(h.stride(1)), self.H, _ptr(self.W), self.H * self.P, _ptr(self.b),
                self.P, self.S)


class BijectorLauncher(_Launcher):
    """Pre-bound one-launch Chain bijector (``nfn_chain_fwd_ldj_f32``) over the layer's
    flow blocks of ``t`` — the Bijector API path (``Chain.forward`` +
    ``forward_log_det_jacobian``) for the benchmark: ``launch()`` writes ``z_out`` (B, d)
    and ``ldj`` (B,)."""

    def __init__(self, z: torch.Tensor, t: torch.Tensor, flow_types: Sequence[str], n_dims: int,
                 trainable_base: bool):
        super().__init__()
        d = int(n_dims)
        self.B = self._check_rows(z, d, t, total_param_size(flow_types, d, trainable_base))
        offs = flow_block_offsets(flow_types, d, trainable_base)
        self.z, self.t = z, t
        self.z_out = torch.empty((self.B, d), dtype=torch.float32, device=z.device)
        self.ldj = torch.empty((self.B,), dtype=torch.float32, device=z.device)
        self._ids, k = flow_ids(flow_types)
        self._offs = (ctypes.c_int32 * max(1, len(offs)))(*offs)
        self._bind("nfn_chain_fwd_ldj_f32", _ptr(z), _row_stride(z), _ptr(t), _row_stride(t), self.B, d,
                   ctypes.cast(self._ids, ctypes.c_void_p), ctypes.cast(self._offs, ctypes.c_void_p), k,
                   _ptr(self.z_out), _ptr(self.ldj))


class GridLauncher(_Launcher):
    """Pre-bound density grid (``nfn_chain_logprob_grid_f32``) for the benchmark: the
    ``log_prob`` of each of G grid values under each of B parameter rows, (G, B) out — the
    evaluation ``flow_plotting.plot_model`` makes (``evaluation/visualization/flow_plotting.py:33-53``)."""

    def __init__(self, y_grid: torch.Tensor, t: torch.Tensor, flow_types: Sequence[str], n_dims: int,
                 trainable_base: bool):
        super().__init__()
        d = int(n_dims)
        self._check_rows(y_grid, d, t, total_param_size(flow_types, d, trainable_base))
        self.G, self.B = int(y_grid.shape[0]), int(t.shape[0])
        self.y_grid, self.t = y_grid, t
        self.out = torch.empty((self.G, self.B), dtype=torch.float32, device=t.device)
        self._ids, k = flow_ids(flow_types)
        self._bind("nfn_chain_logprob_grid_f32", _ptr(y_grid), int(y_grid.stride(0)) if self.G > 1 else 0, self.G,
                   _ptr(t), _row_stride(t), self.B, d, ctypes.cast(self._ids, ctypes.c_void_p), k,
                   int(bool(trainable_base)), None, None, _ptr(self.out), self.B)


class FlowsLauncher(_Launcher):
    """Pre-bound flow-by-flow Bijector path for the benchmark: the Chain's K flows as K
    single-flow launches (``nfn_flow_fwd_ldj_f32``, PlanarFlow.py:68-80 / RadialFlow.py:50-70 /
    AffineFlow.py called one bijector at a time), flow k reading its own parameters and the
    previous flow's z, writing z and its own log|det J| (``ldj`` (K, B)).  ``z_out`` holds
    z_K after ``launch()``.  ``params`` says where the parameters come from:

    * ``"views"`` (what ``normalizing_flows`` does for the flows of one layer's ``t``): when
      ``split_pays`` (narrow blocks in wide rows, e.g. C2) each ``launch()`` first makes the
      flows' blocks contiguous in ONE pass over ``t`` (``nfn_split_blocks_f32``, as TF's slices
      copy them), then runs the K launches on the contiguous blocks; otherwise (C3) the
      launches read their blocks from the rows (``mode`` becomes ``"strided"``);
    * ``"separate"``: the flows were built individually, each over its own contiguous
      (B, param_size) tensor (copied here, once, outside the timed launches);
    * ``"strided"``: each launch reads its block straight from the wide rows of ``t``
      (every launch then fetches the whole 128-B lines: the pre-split path, for the record)."""

    def __init__(self, z: torch.Tensor, t: torch.Tensor, flow_types: Sequence[str], n_dims: int,
                 trainable_base: bool, separate: bool = False, params: Optional[str] = None):
        super().__init__()
        dev = z.device
        d = int(n_dims)
        self.mode = params or ("separate" if separate else "views")
        assert self.mode in ("views", "separate", "strided")
        P = total_param_size(flow_types, d, trainable_base)
        self.B = B = self._check_rows(z, d, t, P)
        K = len(flow_types)
        widths = [param_size(f, d) for f in flow_types]
        offs = flow_block_offsets(flow_types, d, trainable_base)
        zs = [torch.empty((B, d), dtype=torch.float32, device=dev) for _ in range(2)]
        self.ldj = torch.empty((max(1, K), B), dtype=torch.float32, device=dev)
        self.z_out = zs[(K - 1) % 2] if K else z
        self.params = []  # the flows' contiguous parameter tensors (kept alive here)
        if self.mode == "views" and not split_pays(widths, _row_stride(t) or P):
            self.mode = "strided"  # the package's flows read such blocks straight from the rows
        if self.mode != "strided" and K:
            # blocks in row order: flow K-1 first (the layer's reversed layout)
            order = sorted(range(K), key=lambda k: offs[k])
            row_widths = [widths[k] for k in order]
            tb = t[:, P - sum(widths):]  # the flows' columns follow the base's
            blocks = split_blocks(tb, row_widths)
            if self.mode == "views":
                self._bind("nfn_split_blocks_f32", _ptr(tb), _row_stride(tb), B,
                           (ctypes.c_int32 * K)(*row_widths), K, _ptr(blocks[0]))
            by_flow = {k: blocks[i] for i, k in enumerate(order)}
            self.params = [by_flow[k] for k in range(K)]
        zin = z
        for k, f in enumerate(flow_types):
            zo = zs[k % 2]
            if self.mode == "strided":
                pptr, pstride = _ptr(t) + 4 * offs[k], _row_stride(t)
            else:
                pptr, pstride = _ptr(self.params[k]), widths[k]
            self._bind("nfn_flow_fwd_ldj_f32", FLOW_IDS[f], _ptr(zin), _row_stride(zin), pptr, pstride, B, d,
                       _ptr(zo), _ptr(self.ldj[k]))
            zin = zo
        self.bytes_per_launch = float(B) * sum(4 * d + 4 * w + 4 * d + 4 for w in widths)


class ChainLauncher(_SumLauncher):
    """Pre-bound fused-chain launch for repeated evaluation of fixed device
    buffers (the benchmark / serving loop): all validation and pointer
    marshalling happens once; ``launch()`` is a single C-ABI call.

    ``launch()`` writes ``out`` (B,) and ``sum2`` = {fp64 sum, non-finite count}, finished
    in the kernel by its last workgroup (``sum`` is ``sum2[0:1]``)."""

    def __init__(self, y: torch.Tensor, t: torch.Tensor, flow_types: Sequence[str], n_dims: int,
                 trainable_base: bool, write_values: bool = True, draws: Optional[int] = None,
                 fused_sum: bool = True):
        super().__init__()
        self.n_dims = int(n_dims)
        self.P = total_param_size(flow_types, n_dims, trainable_base)
        self.posterior = draws is not None
        if self.posterior:
            assert y.dim() == 2 and y.shape[1] == n_dims and y.stride(1) == 1
            assert t.dim() == 3 and t.shape[0] == draws and t.shape[2] == self.P and t.stride(2) == 1
            self.B = max(int(y.shape[0]), int(t.shape[1]))
            entry, sizes = "nfn_posterior_lse_f32", self.lib.nfn_posterior_workspace_doubles
            rows = (_ptr(t), int(t.stride(0)), 0 if t.shape[1] == 1 else int(t.stride(1)), int(draws))
        else:
            self.B = self._check_rows(y, n_dims, t, self.P)
            entry, sizes = "nfn_chain_logprob_f32", self.lib.nfn_chain_workspace_doubles
            rows = (_ptr(t), _row_stride(t))
        self.y, self.t = y, t
        self.fused_sum = fused_sum
        self._ids, k = flow_ids(flow_types)
        self._bind_sums(entry, _ptr(y), _row_stride(y), *rows, self.B, self.n_dims,
                        ctypes.cast(self._ids, ctypes.c_void_p), k, int(bool(trainable_base)), None, None,
                        n_partials=sizes(self.B, self.n_dims, self.P), write_values=write_values,
                        fused_sum=fused_sum)
        self._reduce = _Launcher()
        self._reduce._bind("nfn_reduce_partials_f64", _ptr(self.partials), _ptr(self.sum2))

    def bind_sum(self, target: torch.Tensor) -> None:
        """Make later launches finish their ``{sum, non-finite count}`` into ``target[0:2]``
        (fp64, device) — e.g. straight into an all-reduce buffer, so a multi-GPU step needs
        no copy kernels between the chain kernel and the collective."""
        assert self.fused_sum, "bind_sum needs the in-kernel finish"
        assert target.dtype == torch.float64 and target.is_contiguous() and target.numel() >= 2
        fn, args, entry = self._calls[0]
        self._calls[0] = (fn, args[:self._sum_at] + (_ptr(target),) + args[self._sum_at + 1:], entry)
        self.sum2, self.sum = target[0:2], target[0:1]

    def finish_sum(self, stream: Optional[int] = None) -> torch.Tensor:
        """``sum`` (1,) fp64 of the last launch: finished inside the kernel by default; with
        ``fused_sum=False`` the launch writes only the partials and this reduces them
        (``nfn_reduce_partials_f64``, the same summation order and bits)."""
        if not self.fused_sum:
            self._reduce.launch(stream)
        return self.sum


class GradLauncher(_Launcher):
    """Pre-bound fused-backward launch over fixed device buffers (the training-step
    benchmark): ``launch()`` writes ``grad_t`` (B, P) and ``grad_y`` (B, d) for the
    upstream gradient ``g_out`` (B,) — one C-ABI call."""

    def __init__(self, y: torch.Tensor, t: torch.Tensor, flow_types: Sequence[str], n_dims: int,
                 trainable_base: bool, g_out: Optional[torch.Tensor] = None, write_logp: bool = False):
        super().__init__()
        dev = y.device
        self.n_dims = int(n_dims)
        self.P = total_param_size(flow_types, n_dims, trainable_base)
        self.B = self._check_rows(y, n_dims, t, self.P)
        assert g_out is None or (g_out.numel() == self.B and g_out.is_contiguous())
        self.y, self.t, self.g_out = y, t, g_out
        self.logp = torch.empty((self.B,), dtype=torch.float32, device=dev) if write_logp else None
        self.grad_t = torch.empty((self.B, self.P), dtype=torch.float32, device=dev)
        self.grad_y = torch.empty((self.B, self.n_dims), dtype=torch.float32, device=dev)
        self._ids, k = flow_ids(flow_types)
        self._bind("nfn_chain_logprob_grad_f32", _ptr(y), _row_stride(y), _ptr(t), _row_stride(t), self.B,
                   self.n_dims, ctypes.cast(self._ids, ctypes.c_void_p), k, int(bool(trainable_base)), None, None,
                   _ptr(g_out), _ptr(self.logp), _ptr(self.grad_t), self.P, _ptr(self.grad_y))


class DenseGradLauncher(_Launcher):
    """Pre-bound fused backward through the output Dense layer
    (``nfn_chain_logprob_dense_grad_f32``) over fixed device buffers (the training-step
    benchmark): ``launch()`` writes ``grad_h`` (B, H), ``grad_W`` (H, P), ``grad_b`` (P,)
    and ``grad_y`` (B, d) for the upstream gradient ``g_out`` — one C-ABI call (the
    fused kernel + the fixed-order partials sum)."""

    def __init__(self, y: torch.Tensor, h: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
                 flow_types: Sequence[str], n_dims: int, trainable_base: bool, g_out: Optional[torch.Tensor] = None):
        super().__init__()
        dev = y.device
        self.n_dims = int(n_dims)
        self.P = total_param_size(flow_types, n_dims, trainable_base)
        self.B, self.H = int(h.shape[0]), int(h.shape[1])
        assert dense_fusable(self.H, self.P, self.n_dims) and h.stride(1) == 1 and h.stride(0) % 4 == 0
        assert tuple(W.shape) == (self.H, self.P) and y.dim() == 2 and y.shape[1] == n_dims
        assert g_out is None or (g_out.numel() == self.B and g_out.is_contiguous())
        self.y, self.h, self.W, self.b, self.g_out = y, h, W.contiguous(), b, g_out
        self.grad_h = torch.empty((self.B, self.H), dtype=torch.float32, device=dev)
        self.grad_W = torch.empty((self.H, self.P), dtype=torch.float32, device=dev)
        self.grad_b = torch.empty((self.P,), dtype=torch.float32, device=dev)
        self.grad_y = torch.empty((self.B, self.n_dims), dtype=torch.float32, device=dev)
        self.ws = torch.empty((max(1, int(self.lib.nfn_dense_grad_workspace_floats(self.B, self.H, self.P))),),
                              dtype=torch.float32, device=dev)
        self._ids, k = flow_ids(flow_types)
        self._bind("nfn_chain_logprob_dense_grad_f32", _ptr(y), _row_stride(y), _ptr(h), int(h.stride(0)), self.H,
                   _ptr(self.W), _ptr(b), self.B, self.n_dims, ctypes.cast(self._ids, ctypes.c_void_p), k,
                   int(bool(trainable_base)), None, None, _ptr(g_out), None, _ptr(self.grad_h), self.H,
                   _ptr(self.grad_W), _ptr(self.grad_b), _ptr(self.grad_y), _ptr(self.ws))


# ---------------------------------------------------------------------------
# Kernel mixture network: Gaussian-kernel mixture log_prob (nfn_mixture.hip)
# ---------------------------------------------------------------------------

def _kernel_params(locs, scales, device):
    """``(locs (M, d), scales (M,), M, d)`` in the C ABI's conventions (both contiguous)."""
    locs = as_device_f32(locs, device)
    assert locs.dim() == 2, "locs must be (M, n_dims)"
    locs = locs.contiguous()
    M, d = int(locs.shape[0]), int(locs.shape[1])
    scales = as_device_f32(scales, device).reshape(-1).contiguous()
    assert scales.numel() == M, f"scales must have {M} elements"
    return locs, scales, M, d


def kernel_mixture_log_prob(y, logits, locs, scales, y_mean=None, y_std=None, want_values: bool = True,
                            want_nonfinite: bool = False, want_sum: bool = False):
    """``log_prob(y)`` of the kernel mixture network's density (``GaussianKernelsLayer``,
    ``DistributionLayers.py:118-133``) in one fused pass over the logits:
    ``logsumexp_k(logits + c) - logsumexp_k(logits)`` with ``c_k`` the log-density of kernel
    ``k`` (centre ``locs[k]``, bandwidth ``scales[k]``, ``|s|`` in the log term only —
    include/nfn.h).  Returns as :func:`chain_log_prob`: ``(log_prob | None, sum | None)``,
    plus the non-finite count with ``want_nonfinite``."""
    dev = _device()
    locs, scales, M, d = _kernel_params(locs, scales, dev)
    y, logits, rs, ym, ys, B = _row_inputs(y, logits, M, d, y_mean, y_std, dev, "logits")
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite or not want_values,
                                 lambda: lib.nfn_kernel_mixture_workspace_doubles(B, d, M), dev)
    rc = lib.nfn_kernel_mixture_logprob_f32(
        _ptr(y), _row_stride(y), _ptr(logits), rs, _ptr(locs), _ptr(scales), B, d, M, _ptr(ym), _ptr(ys),
        _ptr(out), _ptr(osum), _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_kernel_mixture_logprob_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def kernel_mixture_log_prob_grad(y, logits, locs, scales, y_mean=None, y_std=None, g_out=None,
                                 want_logp: bool = False, want_grad_logits: bool = True, want_grad_y: bool = True,
                                 want_grad_scales: bool = True):
    """Fused backward of :func:`kernel_mixture_log_prob` for ``L = sum_b g_out[b] * log_prob_b``
    (``g_out`` None => ones): ``(log_prob | None, dL/dlogits (B, M), dL/dy (B, d), dL/dscales
    (M,))``.  ``dL/dscales`` is a batch sum: per-workgroup partials and a fixed-order final
    sum, so the same inputs give the same bits."""
    dev = _device()
    locs, scales, M, d = _kernel_params(locs, scales, dev)
    y, logits, rs, ym, ys, B = _row_inputs(y, logits, M, d, y_mean, y_std, dev, "logits")
    g = _upstream(g_out, B, dev)
    lp = torch.empty((B,), dtype=torch.float32, device=dev) if want_logp else None
    gl = torch.empty((B, M), dtype=torch.float32, device=dev) if want_grad_logits else None
    gy = torch.empty((B, d), dtype=torch.float32, device=dev) if want_grad_y else None
    gs = torch.empty((M,), dtype=torch.float32, device=dev) if want_grad_scales else None
    lib = _lib.load()
    ws = None
    if want_grad_scales:  # a float view of the stream's (pinned while capturing) workspace
        nfl = int(lib.nfn_kernel_mixture_grad_workspace_floats(B, d, M))
        ws = _workspace((nfl + 1) // 2, dev).view(torch.float32)
    rc = lib.nfn_kernel_mixture_logprob_grad_f32(
        _ptr(y), _row_stride(y), _ptr(logits), rs, _ptr(locs), _ptr(scales), B, d, M, _ptr(ym), _ptr(ys), _ptr(g),
        _ptr(lp), _ptr(gl), M, _ptr(gy), _ptr(gs), _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_kernel_mixture_logprob_grad_f32")
    return lp, gl, gy, gs


class _KernelMixtureLogProb(torch.autograd.Function):
    """The mixture ``log_prob`` as a differentiable op: forward and backward are the two fused
    kernels (nothing but the inputs is saved)."""

    @staticmethod
    def forward(ctx, y, logits, locs, scales, y_mean, y_std):
        out, _ = kernel_mixture_log_prob(y, logits, locs, scales, y_mean, y_std)
        ctx.save_for_backward(y, logits, locs, scales)
        ctx.meta = (y_mean, y_std)
        return out

    @staticmethod
    def backward(ctx, g):
        y, logits, locs, scales = ctx.saved_tensors
        y_mean, y_std = ctx.meta
        need_y, need_l, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        _, gl, gy, gs = kernel_mixture_log_prob_grad(y, logits, locs, scales, y_mean, y_std, g_out=g.contiguous(),
                                                     want_grad_logits=need_l, want_grad_y=need_y,
                                                     want_grad_scales=need_s)
        B = g.shape[0]
        return _unbroadcast(gy, y, B), _unbroadcast(gl, logits, B), None, gs, None, None


def kernel_mixture_log_prob_diff(y, logits, locs, scales, y_mean=None, y_std=None):
    """Differentiable fused mixture ``log_prob`` (B,): gradients w.r.t. ``logits``, ``scales``
    and ``y`` come from the fused backward kernel."""
    dev = _device()
    locs, scales, M, d = _kernel_params(locs, scales, dev)
    y = _prep_2d(y, d, "y", dev)
    logits = _prep_2d(logits, M, "logits", dev)
    y_mean, y_std = _norm_stats(y_mean, y_std, d, dev)
    return _KernelMixtureLogProb.apply(y, logits, locs, scales, y_mean, y_std)


# ---------------------------------------------------------------------------
# Mixture density network: Gaussian-mixture log_prob (nfn_gmm.hip)
# ---------------------------------------------------------------------------

def gaussian_mixture_log_prob(y, t, n_centers, n_dims, y_mean=None, y_std=None, want_values: bool = True,
                              want_nonfinite: bool = False, want_sum: bool = False):
    """``log_prob(y)`` of the mixture density network's density (``GaussianMixtureLayer``,
    ``DistributionLayers.py:174-212``) in one fused pass over the parameter rows ``t``
    ``[loc_0 | raw_0 | ... | loc_{K-1} | raw_{K-1} | logits]`` (include/nfn.h).  Returns as
    :func:`chain_log_prob`: ``(log_prob | None, sum | None)``, plus the non-finite count with
    ``want_nonfinite``."""
    dev = _device()
    K, d = int(n_centers), int(n_dims)
    y, t, rs, ym, ys, B = _row_inputs(y, t, K * (2 * d + 1), d, y_mean, y_std, dev, "t")
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite or not want_values,
                                 lambda: lib.nfn_gaussian_mixture_workspace_doubles(B, d, K), dev)
    rc = lib.nfn_gaussian_mixture_logprob_f32(
        _ptr(y), _row_stride(y), _ptr(t), rs, B, d, K, _ptr(ym), _ptr(ys), _ptr(out), _ptr(osum), _ptr(ws),
        _stream(),
    )
    _lib.check(rc, "nfn_gaussian_mixture_logprob_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def gaussian_mixture_log_prob_grad(y, t, n_centers, n_dims, y_mean=None, y_std=None, g_out=None,
                                   want_logp: bool = False, want_grad_t: bool = True, want_grad_y: bool = True):
    """Fused backward of :func:`gaussian_mixture_log_prob` for ``L = sum_b g_out[b] *
    log_prob_b`` (``g_out`` None => ones): ``(log_prob | None, dL/dt (B, P), dL/dy (B, d))``."""
    dev = _device()
    K, d = int(n_centers), int(n_dims)
    P = K * (2 * d + 1)
    y, t, rs, ym, ys, B = _row_inputs(y, t, P, d, y_mean, y_std, dev, "t")
    g = _upstream(g_out, B, dev)
    lp = torch.empty((B,), dtype=torch.float32, device=dev) if want_logp else None
    gt = torch.empty((B, P), dtype=torch.float32, device=dev) if want_grad_t else None
    gy = torch.empty((B, d), dtype=torch.float32, device=dev) if want_grad_y else None
    rc = _lib.load().nfn_gaussian_mixture_logprob_grad_f32(
        _ptr(y), _row_stride(y), _ptr(t), rs, B, d, K, _ptr(ym), _ptr(ys), _ptr(g), _ptr(lp), _ptr(gt), P,
        _ptr(gy), _stream(),
    )
    _lib.check(rc, "nfn_gaussian_mixture_logprob_grad_f32")
    return lp, gt, gy


class _GaussianMixtureLogProb(torch.autograd.Function):
    """The Gaussian-mixture ``log_prob`` as a differentiable op: forward and backward are the
    two fused kernels (nothing but the inputs is saved)."""

    @staticmethod
    def forward(ctx, y, t, n_centers, n_dims, y_mean, y_std):
        out, _ = gaussian_mixture_log_prob(y, t, n_centers, n_dims, y_mean, y_std)
        ctx.save_for_backward(y, t)
        ctx.meta = (n_centers, n_dims, y_mean, y_std)
        return out

    @staticmethod
    def backward(ctx, g):
        y, t = ctx.saved_tensors
        n_centers, n_dims, y_mean, y_std = ctx.meta
        need_y, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        _, gt, gy = gaussian_mixture_log_prob_grad(y, t, n_centers, n_dims, y_mean, y_std, g_out=g.contiguous(),
                                                   want_grad_t=need_t, want_grad_y=need_y)
        B = g.shape[0]
        return _unbroadcast(gy, y, B), _unbroadcast(gt, t, B), None, None, None, None


def gaussian_mixture_log_prob_diff(y, t, n_centers, n_dims, y_mean=None, y_std=None):
    """Differentiable fused Gaussian-mixture ``log_prob`` (B,): gradients w.r.t. ``t`` and
    ``y`` come from the fused backward kernel."""
    dev = _device()
    K, d = int(n_centers), int(n_dims)
    y = _prep_2d(y, d, "y", dev)
    t = _prep_2d(t, K * (2 * d + 1), "t", dev)
    y_mean, y_std = _norm_stats(y_mean, y_std, d, dev)
    return _GaussianMixtureLogProb.apply(y, t, K, d, y_mean, y_std)


# ---------------------------------------------------------------------------
# Posterior scores of the two mixture layers (BayesianNNEstimator.score)
# ---------------------------------------------------------------------------

def _draw_inputs(y, draws, width: int, n_dims: int, y_mean, y_std, device, name: str):
    """``(y, draws, draw stride, row stride, y_mean, y_std, S, B)`` of a mixture posterior
    entry: ``draws`` (S, B, width) with a unit column stride, its draw and row strides taken
    from the tensor (a column view or a row slice of a larger tensor stays a view); ``y``
    (B or 1, d).  The ABI's rows do not broadcast and have a stride >= width: anything else
    is materialised."""
    y = _prep_2d(y, n_dims, "y", device)
    draws = as_device_f32(draws, device)
    assert draws.dim() == 3 and draws.shape[-1] == width, f"{name} must be (S, B, {width})"
    S, Bt = int(draws.shape[0]), int(draws.shape[1])
    assert S >= 1, "number of draws must be >= 1"
    B = max(int(y.shape[0]), Bt)
    assert y.shape[0] in (1, B) and Bt in (1, B), "incompatible batch sizes"
    if Bt != B:
        draws = draws.expand(S, B, width).contiguous()
    if draws.stride(-1) != 1 or (B > 1 and draws.stride(1) < width):
        draws = draws.contiguous()
    ds = int(draws.stride(0)) if S > 1 else 0
    rs = int(draws.stride(1)) if B > 1 else width
    return (y, draws, ds, rs) + _norm_stats(y_mean, y_std, n_dims, device) + (S, B)


def posterior_lse_gaussian_mixture(y, t_draws, n_centers, n_dims, y_mean=None, y_std=None, want_values: bool = True,
                                   want_sum: bool = False, want_nonfinite: bool = False):
    """``logsumexp_s(log_pdf(y_b | t[s, b])) - log S`` per sample under the mixture density
    network's density (``BayesianNNEstimator.py:65-76`` over a ``GaussianMixtureLayer``), in
    ONE fused kernel: ``y`` is read once, the running log-sum-exp stays in registers and one
    float per sample is written.  ``t_draws``: (S, B, K (2 d + 1)).  A draw whose logits are all
    ``-inf`` counts as a ``-inf`` term and drops out (include/nfn.h).  Returns as
    :func:`posterior_lse`; not differentiable."""
    dev = _device()
    K, d = int(n_centers), int(n_dims)
    y, t, ds, rs, ym, ys, S, B = _draw_inputs(y, t_draws, K * (2 * d + 1), d, y_mean, y_std, dev, "t_draws")
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite or not want_values,
                                 lambda: lib.nfn_posterior_gaussian_mixture_workspace_doubles(B, d, K), dev)
    rc = lib.nfn_posterior_lse_gaussian_mixture_f32(
        _ptr(y), _row_stride(y), _ptr(t), ds, rs, S, B, d, K, _ptr(ym), _ptr(ys), _ptr(out), _ptr(osum), _ptr(ws),
        _stream(),
    )
    _lib.check(rc, "nfn_posterior_lse_gaussian_mixture_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


def posterior_lse_kernel_mixture(y, logits_draws, locs, scales, y_mean=None, y_std=None, want_values: bool = True,
                                 want_sum: bool = False, want_nonfinite: bool = False):
    """``logsumexp_s(log_pdf(y_b | logits[s, b])) - log S`` per sample under the kernel mixture
    network's density (``BayesianNNEstimator.py:65-76`` over a ``GaussianKernelsLayer``), in
    ONE fused kernel: the kernel terms ``c_bk`` (a function of ``y_b`` and the fixed centres
    only) are formed once per row, not once per draw.  ``logits_draws``: (S, B, M).  A draw whose
    logits are all ``-inf`` counts as a ``-inf`` term and drops out (include/nfn.h).  Returns as
    :func:`posterior_lse`; not differentiable."""
    dev = _device()
    locs, scales, M, d = _kernel_params(locs, scales, dev)
    y, lg, ds, rs, ym, ys, S, B = _draw_inputs(y, logits_draws, M, d, y_mean, y_std, dev, "logits_draws")
    lib = _lib.load()
    out, osum, ws = _sum_outputs(B, want_values, want_sum or want_nonfinite or not want_values,
                                 lambda: lib.nfn_posterior_kernel_mixture_workspace_doubles(B, d, M), dev)
    rc = lib.nfn_posterior_lse_kernel_mixture_f32(
        _ptr(y), _row_stride(y), _ptr(lg), ds, rs, S, _ptr(locs), _ptr(scales), B, d, M, _ptr(ym), _ptr(ys),
        _ptr(out), _ptr(osum), _ptr(ws), _stream(),
    )
    _lib.check(rc, "nfn_posterior_lse_kernel_mixture_f32")
    return _with_nonfinite(out, osum, want_nonfinite)


# ---------------------------------------------------------------------------
# Variational training: the mean-field draw and KL(q || p) (nfn_meanfield.hip)
# ---------------------------------------------------------------------------

def _numel(x) -> int:
    return int(x.numel()) if isinstance(x, torch.Tensor) else int(np.size(x))


def _flat(x, device) -> Optional[torch.Tensor]:
    """A flat fp32 device vector (a contiguous view stays a view), or None."""
    return None if x is None else as_device_f32(x, device).reshape(-1)


def _mean_field_inputs(loc, rho, eps, prior_loc, prior_scale, **more):
    """``(loc, rho, eps, prior_loc, N, device, more)`` as flat device vectors of one length.
    ``rho`` and ``eps`` are both None in map mode.  The lengths are checked before anything
    touches the device."""
    N = _numel(loc)
    assert (rho is None) == (eps is None), "rho and eps must both be given or both None (map mode)"
    for name, v in dict(rho=rho, eps=eps, prior_loc=prior_loc, **more).items():
        assert v is None or _numel(v) == N, f"{name} must have {N} elements like loc, got {_numel(v)}"
    assert float(prior_scale) > 0.0 and np.isfinite(float(prior_scale)), "prior_scale must be > 0 and finite"
    dev = _device()
    return (_flat(loc, dev), _flat(rho, dev), _flat(eps, dev), _flat(prior_loc, dev), N, dev,
            {k: _flat(v, dev) for k, v in more.items()})


def mean_field_draw_kl(loc, rho, eps, prior_loc=None, prior_scale: float = 1.0, kl_exact: bool = True,
                       want_w: bool = True, want_kl: bool = True):
    """One draw ``w = loc + s * eps`` of the mean-field posterior over a flat vector of weights,
    ``s = 1e-3 + softplus(log(e - 1) + 0.05 rho)`` (``MeanFieldLayer``,
    ``DistributionLayers.py:17-71``), and KL(q || p) against ``Normal(prior_loc or 0,
    prior_scale)`` in the same launch: the closed form with ``kl_exact``, else ``log q(w) -
    log p(w)`` at that draw (``DenseVariational``'s ``kl_use_exact``).  ``rho = eps = None`` is
    map mode (include/nfn.h).  Returns ``(w | None, kl_pair | None)``; ``kl_pair`` is the
    kernel's (2,) fp64 {KL, number of non-finite terms}."""
    loc, rho, eps, prior_loc, N, dev, _ = _mean_field_inputs(loc, rho, eps, prior_loc, prior_scale)
    assert want_w or want_kl, "neither w nor kl requested"
    lib = _lib.load()
    w, kl, ws = _sum_outputs(N, want_w, want_kl, lambda: lib.nfn_mean_field_workspace_doubles(N), dev)
    rc = lib.nfn_mean_field_draw_kl_f32(_ptr(loc), _ptr(rho), _ptr(eps), _ptr(prior_loc), float(prior_scale), N,
                                        int(bool(kl_exact)), _ptr(w), _ptr(kl), _ptr(ws), _stream())
    _lib.check(rc, "nfn_mean_field_draw_kl_f32")
    return w, kl


def mean_field_draw_kl_grad(loc, rho, eps, prior_loc=None, prior_scale: float = 1.0, kl_exact: bool = True,
                            g_w=None, g_kl=None, want_grad_prior: bool = False):
    """Backward of :func:`mean_field_draw_kl` for the upstream gradients ``g_w`` (of the draw,
    None = 0) and ``g_kl`` (of the KL sum: a one-element device tensor or a number, None = 0):
    ``(grad_loc, grad_rho | None in map mode, grad_prior_loc | None)``, one launch, no
    reduction."""
    loc, rho, eps, prior_loc, N, dev, more = _mean_field_inputs(loc, rho, eps, prior_loc, prior_scale, g_w=g_w)
    if g_kl is not None:
        g_kl = as_device_f32(g_kl, dev).reshape(-1)
        assert g_kl.numel() == 1, "g_kl must have one element"
    g_loc = torch.empty((N,), dtype=torch.float32, device=dev)
    g_rho = torch.empty((N,), dtype=torch.float32, device=dev) if rho is not None else None
    g_prior = torch.empty((N,), dtype=torch.float32, device=dev) if want_grad_prior else None
    rc = _lib.load().nfn_mean_field_draw_kl_grad_f32(
        _ptr(loc), _ptr(rho), _ptr(eps), _ptr(prior_loc), float(prior_scale), N, int(bool(kl_exact)),
        _ptr(more["g_w"]), _ptr(g_kl), _ptr(g_loc), _ptr(g_rho), _ptr(g_prior), _stream())
    _lib.check(rc, "nfn_mean_field_draw_kl_grad_f32")
    return g_loc, g_rho, g_prior


class _MeanFieldDrawKL(torch.autograd.Function):
    """The draw and its KL as a differentiable op: forward and backward are the two fused
    kernels (nothing but the inputs is saved)."""

    @staticmethod
    def forward(ctx, loc, rho, eps, prior_loc, prior_scale, kl_exact):
        w, kl = mean_field_draw_kl(loc, rho, eps, prior_loc, prior_scale, kl_exact)
        ctx.save_for_backward(loc, rho, eps, prior_loc)
        ctx.meta = (prior_scale, kl_exact)
        return w, kl[0].float()

    @staticmethod
    def backward(ctx, g_w, g_kl):
        loc, rho, eps, prior_loc = ctx.saved_tensors
        prior_scale, kl_exact = ctx.meta
        need_prior = prior_loc is not None and ctx.needs_input_grad[3]
        g_loc, g_rho, g_prior = mean_field_draw_kl_grad(loc, rho, eps, prior_loc, prior_scale, kl_exact, g_w=g_w,
                                                        g_kl=g_kl, want_grad_prior=need_prior)
        return g_loc, g_rho, None, g_prior, None, None


def mean_field_draw_kl_diff(loc, rho, eps, prior_loc=None, prior_scale: float = 1.0, kl_exact: bool = True):
    """Differentiable :func:`mean_field_draw_kl`: ``(w (N,), kl)`` with ``kl`` a device fp32
    scalar; the gradients w.r.t. ``loc``, ``rho`` and ``prior_loc`` come from the fused backward
    kernel (``eps`` is a constant of the draw)."""
    loc, rho, eps, prior_loc, _, _, _ = _mean_field_inputs(loc, rho, eps, prior_loc, prior_scale)
    return _MeanFieldDrawKL.apply(loc, rho, eps, prior_loc, float(prior_scale), bool(kl_exact))
