"""The middle of a PTv3 Block over libgcm_hip.so (include/gcm.h): what SerializedAttention.forward
runs around its attention, and the Block's DropPath and residual add after it.

  slot_plan(order [T], inverse [N], check=False) -> extra [N] int32
        extra[n] is the duplicate slot of row n (a slot j != inverse[n] with order[j] == n), or -1.  The data operators
        rely on the precondition order[inverse[n]] == n and at most one duplicate slot per row, which
        get_padding_and_inverse's index pairs meet; check=True verifies it with one host wait and raises.
  gather_rows(x [N, W], order, inverse, extra) -> [T, W]
        x[order]; its gradient is dy[inverse] + dy[extra], one writer per element and no sort, bit-identical to torch's.
  proj_residual(a [T, C], inverse, extra, x [N, C], wp [C, C], bp [C], row_scale=None) -> [N, C]
        x + (a[inverse] @ wp.T + bp), or x + (a[inverse] @ wp.T + bp) * row_scale[:, None]: one launch.  Gradients for a
        (written whole: zeros at the duplicate slots), x (the incoming gradient itself), wp and bp, deterministic (no float
        atomics); row_scale, a DropPath mask, gets none.
        Both take extra=None when no gradient is needed (under no_grad, or when no float input requires one): a forward
        alone does not read it, and the caller saves slot_plan's launches.
  max_channels()                  the largest C the fused kernels run
  stats() / reset_stats()

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation is in
the HIP library, float32 throughout, and nothing here waits for the device unless check=True asks for it.
"""
import functools

import torch

from . import _native_m as M
from ._loader import current_stream as _stream
from ._loader import dense as _dense
from .modlinear import _check_float as _check_float_op
from .modlinear import _grad32, _ptr, _rows, _workspace

_check_float = functools.partial(_check_float_op, op=None)  # the device is checked after everything else

_STATS = {"plan_calls": 0, "gather_forward_calls": 0, "gather_backward_calls": 0, "forward_calls": 0, "backward_calls": 0}


def stats():
    """Counters of this process: calls of the library's entry points."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def max_channels():
    """The largest C the library's fused kernels run.  Loads the library."""
    return int(M.lib().gcm_mid_max_channels())


def _check_cuda(name, t):
    if not t.is_cuda:
        raise TypeError("the fused Block middle runs on the GPU; %s must be a CUDA tensor" % name)


def _check_index(name, t, dtype=torch.int64):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1:
        raise TypeError("%s must be a 1-d %s tensor" % (name, str(dtype).replace("torch.", "")))


def _check_pair(order, inverse, extra=None):
    """Types and shapes; the device comes after every other check (_check_cuda_all)."""
    _check_index("order", order)
    _check_index("inverse", inverse)
    if order.shape[0] < inverse.shape[0]:
        raise ValueError("order has %d slots for the %d rows of inverse: T >= N" % (order.shape[0], inverse.shape[0]))
    if extra is not None:
        _check_index("extra", extra, torch.int32)
        if extra.shape != inverse.shape:
            raise ValueError("extra must be %r as inverse, got %r" % (tuple(inverse.shape), tuple(extra.shape)))


def _check_cuda_all(**named):
    for name, t in named.items():
        _check_cuda(name, t)


def slot_plan(order, inverse, check=False):
    """extra [N] int32 from order [T] and inverse [N] (int64 on the GPU, T >= N): the duplicate slot of every row, or -1.
    check=True waits for the device once and raises ValueError, naming the rule, when order[inverse[n]] != n for a row or
    a row has more than one duplicate slot."""
    _check_pair(order, inverse)
    _check_cuda_all(order=order, inverse=inverse)
    order, inverse = order.contiguous(), inverse.contiguous()
    T, N = order.shape[0], inverse.shape[0]
    extra = torch.empty(N, dtype=torch.int32, device=order.device)
    with torch.cuda.device(order.device):
        M.check(M.lib().gcm_mid_slot_plan(order.data_ptr(), T, inverse.data_ptr(), N, extra.data_ptr(), _stream()),
                "gcm_mid_slot_plan")
    _STATS["plan_calls"] += 1
    if check and N:
        dev = order.device
        in_range = ((order >= 0) & (order < N)).all() & ((inverse >= 0) & (inverse < T)).all()
        o, i = order.clamp(0, N - 1), inverse.clamp(0, T - 1)       # what follows indexes with clamped values only
        own = (o[i] == torch.arange(N, device=dev)).all()
        dup = i[o] != torch.arange(T, device=dev)
        most = torch.zeros(N, dtype=torch.int64, device=dev).scatter_add_(0, o, dup.long()).max()
        in_range, own, most = torch.stack([in_range.long(), own.long(), most]).tolist()   # the one wait
        if not in_range:
            raise ValueError("order must hold rows 0 .. N-1 and inverse slots 0 .. T-1")
        if not own:
            raise ValueError("order[inverse[n]] == n does not hold for every row")
        if most > 1:
            raise ValueError("a row has %d duplicate slots: at most one duplicate slot per row" % most)
    return extra


class GatherRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, order, inverse, extra):
        x = _rows(x)
        T, W = order.shape[0], x.shape[1]
        y = x.new_empty((T, W))
        with torch.cuda.device(x.device):
            M.check(M.lib().gcm_mid_gather_forward(x.data_ptr(), x.stride(0), order.data_ptr(), T, W, y.data_ptr(), _stream()),
                    "gcm_mid_gather_forward")
        _STATS["gather_forward_calls"] += 1
        if extra is not None:
            ctx.save_for_backward(inverse, extra)
        return y

    @staticmethod
    def backward(ctx, dy):
        inverse, extra = ctx.saved_tensors
        dy = _grad32(dy)
        N, W = inverse.shape[0], dy.shape[1]
        dx = dy.new_empty((N, W))
        with torch.cuda.device(dy.device):
            M.check(M.lib().gcm_mid_gather_backward(dy.data_ptr(), dy.stride(0), inverse.data_ptr(), extra.data_ptr(), N, W,
                                                    dx.data_ptr(), _stream()), "gcm_mid_gather_backward")
        _STATS["gather_backward_calls"] += 1
        return dx, None, None, None


def _no_plan(*floats):
    """extra=None: fine while nothing asks for a gradient."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in floats):
        raise ValueError("extra (slot_plan) is required when a gradient is: extra=None serves a forward alone")


def gather_rows(x, order, inverse, extra=None):
    """x[order] for x [N, W] float32 on the GPU, W a positive multiple of 4; inverse and extra (slot_plan) serve the
    gradient, and extra may be None when none is needed.  order must hold rows of x only: the library cannot check it
    without a wait."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("x must be [N, W]")
    if extra is None:
        _no_plan(x)
    _check_pair(order, inverse, extra)
    N, W = x.shape
    if W % 4 or W == 0:
        raise ValueError("W must be a positive multiple of 4, got W = %d" % W)
    _check_float("x", x, (inverse.shape[0], W))
    _check_cuda_all(x=x, order=order, inverse=inverse, **({} if extra is None else {"extra": extra}))
    if extra is None:
        with torch.no_grad():
            return GatherRowsFunction.apply(x, order.contiguous(), inverse.contiguous(), None)
    return GatherRowsFunction.apply(x, order.contiguous(), inverse.contiguous(), extra.contiguous())


class ProjResidualFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, inverse, extra, x, wp, bp, row_scale):
        a, x = _rows(a), _rows(x)
        wp, bp = _dense(wp), _dense(bp)
        N, C = x.shape
        y = x.new_empty((N, C))
        with torch.cuda.device(x.device):
            M.check(M.lib().gcm_mid_forward(a.data_ptr(), a.stride(0), inverse.data_ptr(), x.data_ptr(), x.stride(0),
                                            wp.data_ptr(), bp.data_ptr(), _ptr(row_scale), N, C, y.data_ptr(), y.stride(0),
                                            _stream()), "gcm_mid_forward")
        _STATS["forward_calls"] += 1
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(a, inverse, extra, wp, row_scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, inverse, extra, wp, row_scale = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dy if need[3] else None  # the shortcut's gradient is the incoming one
        if not (need[0] or need[4] or need[5]):
            return None, None, None, dx, None, None, None
        g = _grad32(dy)
        (T, C), N = a.shape, inverse.shape[0]
        da = a.new_empty((T, C)) if need[0] else None
        dwp = a.new_empty((C, C)) if need[4] else None
        dbp = a.new_empty((C,)) if need[5] else None
        L = M.lib()
        ws_bytes = L.gcm_mid_backward_workspace_bytes(N, C)
        ws = _workspace(ws_bytes, a.device)
        with torch.cuda.device(a.device):
            M.check(L.gcm_mid_backward(a.data_ptr(), a.stride(0), inverse.data_ptr(), extra.data_ptr(), g.data_ptr(),
                                       g.stride(0), wp.data_ptr(), _ptr(row_scale), N, T, C, _ptr(da), _ptr(dwp), _ptr(dbp),
                                       ws.data_ptr(), ws_bytes, _stream()), "gcm_mid_backward")
        _STATS["backward_calls"] += 1
        return da, None, None, dx, dwp, dbp, None


def proj_residual(a, inverse, extra, x, wp, bp, row_scale=None):
    """x + (a[inverse] @ wp.T + bp) [* row_scale] for a [T, C], x [N, C], wp [C, C], bp [C] float32 on the GPU, inverse [N]
    int64 and extra [N] int32 (slot_plan; None when no gradient is needed), row_scale None or [N] / [N, 1] float32.  C is a
    positive multiple of 4, at most max_channels()."""
    if not isinstance(a, torch.Tensor) or a.dim() != 2 or not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("a must be [T, C] and x [N, C]")
    (T, C), N = a.shape, x.shape[0]
    if C % 4 or C == 0:
        raise ValueError("C must be a positive multiple of 4, got C = %d" % C)
    if C > max_channels():
        raise ValueError("C = %d: the fused kernels hold C up to %d" % (C, max_channels()))
    _check_index("inverse", inverse)
    if extra is None:
        _no_plan(a, x, wp, bp)
    else:
        _check_index("extra", extra, torch.int32)
    if inverse.shape[0] != N or (extra is not None and extra.shape[0] != N) or T < N:
        raise ValueError("inverse and extra must be (%d,) as x has rows, and a must have T >= N rows; got %r, %r and T = %d"
                         % (N, tuple(inverse.shape), None if extra is None else tuple(extra.shape), T))
    _check_float("a", a, (T, C))
    _check_float("x", x, (N, C))
    _check_float("wp", wp, (C, C))
    _check_float("bp", bp, (C,))
    if row_scale is not None:
        if isinstance(row_scale, torch.Tensor) and row_scale.dim() == 2 and row_scale.shape[1] == 1:
            row_scale = row_scale[:, 0]
        _check_float("row_scale", row_scale, (N,))
        row_scale = _dense(row_scale.detach())
    named = {"a": a, "x": x, "wp": wp, "bp": bp, "inverse": inverse, "extra": extra, "row_scale": row_scale}
    _check_cuda_all(**{k: v for k, v in named.items() if v is not None})
    if extra is None:
        with torch.no_grad():
            return ProjResidualFunction.apply(a, inverse.contiguous(), None, x, wp, bp, row_scale)
    return ProjResidualFunction.apply(a, inverse.contiguous(), extra.contiguous(), x, wp, bp, row_scale)
