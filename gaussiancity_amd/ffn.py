"""The feed-forward third of a PTv3 Block over libgcm_hip.so (include/gcm.h).

  layernorm_mlp_residual(x [N, C], ln_weight [C], ln_bias [C], eps, w1 [Hd, C], b1 [Hd], w2 [C, Hd], b2 [C], row_scale)
        y = x + row_scale[:, None] * (gelu(layer_norm(x) @ w1.T + b1) @ w2.T + b2), erf GELU, row_scale [N] or None.
        One launch forward; under no_grad the hidden tensor never reaches memory.  Gradients for x and the six
        parameters, deterministic (no float atomics), from the saved pre-activation [N, Hd], mean and rstd [N].
        split=True: the same operator through gcm_ffn_split_*, whose row-side kernels give each (row tile, chunk of 64
        hidden features) its own workgroup: C up to split_max_channels(), two launches forward; for C <= max_channels()
        the bits are those of the default path.
  max_channels()                  the largest C the fused kernels run (Hd up to four times that)
  split_max_channels()            the same for split=True
  stats() / reset_stats()         calls of the library, both paths;  split_stats(): those of the split path

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation is in
the HIP library, float32 throughout, and nothing here waits for the device.
"""
import ctypes
import functools

import torch

from . import _native_m as M
from ._loader import current_stream as _stream
from ._loader import dense as _dense
from .modlinear import _check_float as _check_float_op
from .modlinear import _grad32, _ptr, _rows, _workspace

_check_float = functools.partial(_check_float_op, op="the fused feed-forward")

_STATS = {"forward_calls": 0, "backward_calls": 0}
_SPLIT_STATS = {"forward_calls": 0, "backward_calls": 0}


def stats():
    """Counters of this process: calls of the two entry points of the library."""
    return dict(_STATS)


def split_stats():
    """The calls among stats() that went through the split entry points."""
    return dict(_SPLIT_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = _SPLIT_STATS[k] = 0


def max_channels():
    """The largest C the library's fused kernels run; Hd may be up to four times that.  Loads the library."""
    return int(M.lib().gcm_ffn_max_channels())


def split_max_channels():
    """The largest C the split entry points run; Hd may be up to four times that.  Loads the library."""
    return int(M.lib().gcm_ffn_split_max_channels())


def split_plan(N, C, Hd):
    """The library's plan for the split entry points: mode ("rows" or "split"), tiles, chunks, records, weight_slices,
    ln_groups and limit (tiles x chunks up to it run in split mode)."""
    plan = (ctypes.c_int64 * 8)()
    M.check(M.lib().gcm_ffn_split_plan(N, C, Hd, plan), "gcm_ffn_split_plan")
    return {"mode": "split" if plan[0] else "rows", "tiles": plan[1], "chunks": plan[2], "records": plan[3],
            "weight_slices": plan[4], "ln_groups": plan[5], "limit": plan[6]}


def _split_bytes(N, C, Hd):
    fwd, bwd = ctypes.c_size_t(), ctypes.c_size_t()
    M.check(M.lib().gcm_ffn_split_workspace_bytes(N, C, Hd, ctypes.byref(fwd), ctypes.byref(bwd)), "gcm_ffn_split_workspace_bytes")
    return fwd.value, bwd.value


class LayerNormMlpResidualFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ln_w, ln_b, eps, w1, b1, w2, b2, row_scale, split=False):
        x = _rows(x)
        ln_w, ln_b, w1, b1, w2, b2 = (_dense(t) for t in (ln_w, ln_b, w1, b1, w2, b2))
        row_scale = None if row_scale is None else _dense(row_scale)
        N, C = x.shape
        Hd = w1.shape[0]
        need = any(ctx.needs_input_grad)
        y = x.new_empty((N, C))
        mean = x.new_empty((N,)) if need else None
        rstd = x.new_empty((N,)) if need else None
        a = x.new_empty((N, Hd)) if need else None
        args = (x.data_ptr(), x.stride(0), ln_w.data_ptr(), ln_b.data_ptr(), eps, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                b2.data_ptr(), _ptr(row_scale), N, C, Hd, y.data_ptr(), y.stride(0), _ptr(mean), _ptr(rstd), _ptr(a))
        with torch.cuda.device(x.device):
            if split:
                ws_bytes = _split_bytes(N, C, Hd)[0]
                ws = _workspace(ws_bytes, x.device)
                M.check(M.lib().gcm_ffn_split_forward(*args, ws.data_ptr(), ws_bytes, _stream()), "gcm_ffn_split_forward")
                _SPLIT_STATS["forward_calls"] += 1
            else:
                M.check(M.lib().gcm_ffn_forward(*args, _stream()), "gcm_ffn_forward")
        _STATS["forward_calls"] += 1
        ctx.split = split
        if need:
            ctx.save_for_backward(x, mean, rstd, a, row_scale, ln_w, ln_b, w1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, a, row_scale, ln_w, ln_b, w1, w2 = ctx.saved_tensors
        N, C = x.shape
        Hd = w1.shape[0]
        dy = _grad32(dy)
        need = ctx.needs_input_grad
        dx = x.new_empty((N, C)) if need[0] else None
        dln_w = x.new_empty((C,)) if need[1] else None
        dln_b = x.new_empty((C,)) if need[2] else None
        dw1 = x.new_empty((Hd, C)) if need[4] else None
        db1 = x.new_empty((Hd,)) if need[5] else None
        dw2 = x.new_empty((C, Hd)) if need[6] else None
        db2 = x.new_empty((C,)) if need[7] else None
        L = M.lib()
        ws_bytes = _split_bytes(N, C, Hd)[1] if ctx.split else L.gcm_ffn_backward_workspace_bytes(N, C, Hd)
        ws = _workspace(ws_bytes, x.device)
        entry, name = (L.gcm_ffn_split_backward, "gcm_ffn_split_backward") if ctx.split else (L.gcm_ffn_backward, "gcm_ffn_backward")
        with torch.cuda.device(x.device):
            M.check(entry(x.data_ptr(), x.stride(0), mean.data_ptr(), rstd.data_ptr(), a.data_ptr(), dy.data_ptr(),
                          dy.stride(0), _ptr(row_scale), ln_w.data_ptr(), ln_b.data_ptr(), w1.data_ptr(),
                          w2.data_ptr(), N, C, Hd, _ptr(dx), C, _ptr(dln_w), _ptr(dln_b), _ptr(dw1), _ptr(db1),
                          _ptr(dw2), _ptr(db2), ws.data_ptr(), ws_bytes, _stream()), name)
        _STATS["backward_calls"] += 1
        if ctx.split:
            _SPLIT_STATS["backward_calls"] += 1
        return dx, dln_w, dln_b, None, dw1, db1, dw2, db2, None, None


def layernorm_mlp_residual(x, ln_weight, ln_bias, eps, w1, b1, w2, b2, row_scale=None, split=False):
    """x + row_scale[:, None] * (gelu(layer_norm(x, (C,), ln_weight, ln_bias, eps) @ w1.T + b1) @ w2.T + b2) for x [N, C],
    w1 [Hd, C], w2 [C, Hd] float32 on the GPU; the GELU is the erf one.  C and Hd are positive multiples of 4, C at most
    max_channels() and Hd at most four times that.  row_scale [N] (or [N, 1]) multiplies the branch per row (DropPath's
    mask); None means ones.  It receives no gradient.  split=True takes the entry points that split the hidden width across
    workgroups: C up to split_max_channels(), and for C up to max_channels() the same bits as the default."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(w1, torch.Tensor) or w1.dim() != 2:
        raise ValueError("x must be [N, C] and w1 [Hd, C]")
    (N, C), Hd = x.shape, w1.shape[0]
    if C % 4 or Hd % 4 or C == 0 or Hd == 0:
        raise ValueError("C and Hd must be positive multiples of 4, got C = %d, Hd = %d" % (C, Hd))
    _check_float("x", x, (N, C))
    _check_float("ln_weight", ln_weight, (C,))
    _check_float("ln_bias", ln_bias, (C,))
    _check_float("w1", w1, (Hd, C))
    _check_float("b1", b1, (Hd,))
    _check_float("w2", w2, (C, Hd))
    _check_float("b2", b2, (C,))
    if row_scale is not None:
        if isinstance(row_scale, torch.Tensor) and tuple(row_scale.shape) == (N, 1):
            row_scale = row_scale.reshape(N)
        _check_float("row_scale", row_scale, (N,))
        row_scale = row_scale.detach()
    limit = split_max_channels() if split else max_channels()
    if C > limit or Hd > 4 * limit:
        raise ValueError("C = %d, Hd = %d: the fused kernels hold C up to %d and Hd up to %d" % (C, Hd, limit, 4 * limit))
    return LayerNormMlpResidualFunction.apply(x, ln_weight, ln_bias, float(eps), w1, b1, w2, b2, row_scale, bool(split))
