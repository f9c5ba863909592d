"""The front of a PTv3 Block over libgcm_hip.so (include/gcm.h): what Block.forward runs between its
sparse convolution and its attention.

  conv_tail_norm_qkv(x [N, C], s [N, C], wc [C, C], bc [C], lnc_w [C], lnc_b [C], lnc_eps, ln1_w [C], ln1_b [C], ln1_eps,
                     wq [O, C], bq [O]) -> (feat [N, C], qkv [N, O])
        feat = x + layer_norm(s @ wc.T + bc, lnc_w, lnc_b, lnc_eps), qkv = layer_norm(feat, ln1_w, ln1_b, ln1_eps) @ wq.T + bq.
        One launch forward; under no_grad nothing but feat and qkv reaches memory.  Gradients for x, s and the eight
        parameters, deterministic (no float atomics), from the saved pre-norm product [N, C] and four statistics [N].
  max_channels()                  the largest C the fused kernels run (O up to three times that)
  stats() / reset_stats()

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation is in
the HIP library, float32 throughout, and nothing here waits for the device.
"""
import functools

import torch

from . import _native_m as M
from ._loader import current_stream as _stream
from ._loader import dense as _dense
from .modlinear import _check_float as _check_float_op
from .modlinear import _grad32, _ptr, _rows, _workspace

_check_float = functools.partial(_check_float_op, op="the fused Block front")

_STATS = {"forward_calls": 0, "backward_calls": 0}


def stats():
    """Counters of this process: calls of the two entry points of the library."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def max_channels():
    """The largest C the library's fused kernels run; O may be up to three times that.  Loads the library."""
    return int(M.lib().gcm_front_max_channels())


class ConvTailNormQkvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, wc, bc, lnc_w, lnc_b, lnc_eps, ln1_w, ln1_b, ln1_eps, wq, bq):
        x, s = _rows(x), _rows(s)
        wc, bc, lnc_w, lnc_b, ln1_w, ln1_b, wq, bq = (_dense(t) for t in (wc, bc, lnc_w, lnc_b, ln1_w, ln1_b, wq, bq))
        N, C = x.shape
        O = wq.shape[0]
        need = any(ctx.needs_input_grad)
        feat, qkv = x.new_empty((N, C)), x.new_empty((N, O))
        t = x.new_empty((N, C)) if need else None
        st = x.new_empty((4, N)) if need else None  # mean_c, rstd_c, mean_1, rstd_1
        with torch.cuda.device(x.device):
            M.check(M.lib().gcm_front_forward(x.data_ptr(), x.stride(0), s.data_ptr(), s.stride(0), wc.data_ptr(), bc.data_ptr(),
                                              lnc_w.data_ptr(), lnc_b.data_ptr(), lnc_eps, ln1_w.data_ptr(), ln1_b.data_ptr(),
                                              ln1_eps, wq.data_ptr(), bq.data_ptr(), N, C, O, feat.data_ptr(), feat.stride(0),
                                              qkv.data_ptr(), qkv.stride(0), _ptr(t), *_stat_ptrs(st), _stream()),
                    "gcm_front_forward")
        _STATS["forward_calls"] += 1
        if need:
            ctx.save_for_backward(s, feat, t, st, wc, lnc_w, ln1_w, ln1_b, wq)
        return feat, qkv

    @staticmethod
    def backward(ctx, dfeat, dqkv):
        s, feat, t, st, wc, lnc_w, ln1_w, ln1_b, wq = ctx.saved_tensors
        N, C = s.shape
        O = wq.shape[0]
        dfeat, dqkv = _grad32(dfeat), _grad32(dqkv)
        need = ctx.needs_input_grad
        new = lambda i, *shape: s.new_empty(shape) if need[i] else None  # noqa: E731
        dx, ds, dwc, dbc, dlnc_w, dlnc_b = new(0, N, C), new(1, N, C), new(2, C, C), new(3, C), new(4, C), new(5, C)
        dln1_w, dln1_b, dwq, dbq = new(7, C), new(8, C), new(10, O, C), new(11, O)
        L = M.lib()
        ws_bytes = L.gcm_front_backward_workspace_bytes(N, C, O)
        ws = _workspace(ws_bytes, s.device)
        with torch.cuda.device(s.device):
            M.check(L.gcm_front_backward(s.data_ptr(), s.stride(0), feat.data_ptr(), feat.stride(0), t.data_ptr(),
                                         *_stat_ptrs(st), dfeat.data_ptr(), dfeat.stride(0), dqkv.data_ptr(), dqkv.stride(0),
                                         wc.data_ptr(), lnc_w.data_ptr(), ln1_w.data_ptr(), ln1_b.data_ptr(), wq.data_ptr(), N, C,
                                         O, _ptr(dx), C, _ptr(ds), C, _ptr(dwc), _ptr(dbc), _ptr(dlnc_w), _ptr(dlnc_b),
                                         _ptr(dln1_w), _ptr(dln1_b), _ptr(dwq), _ptr(dbq), ws.data_ptr(), ws_bytes, _stream()),
                    "gcm_front_backward")
        _STATS["backward_calls"] += 1
        return dx, ds, dwc, dbc, dlnc_w, dlnc_b, None, dln1_w, dln1_b, None, dwq, dbq


def _stat_ptrs(st):
    """The four rows of the statistics tensor [4, N], or four nulls."""
    if st is None:
        return (None,) * 4
    return tuple(st.data_ptr() + 4 * k * st.shape[1] for k in range(4))


def conv_tail_norm_qkv(x, s, wc, bc, lnc_w, lnc_b, lnc_eps, ln1_w, ln1_b, ln1_eps, wq, bq):
    """(feat, qkv) with feat = x + layer_norm(s @ wc.T + bc, (C,), lnc_w, lnc_b, lnc_eps) and
    qkv = layer_norm(feat, (C,), ln1_w, ln1_b, ln1_eps) @ wq.T + bq, for x, s [N, C], wc [C, C] and wq [O, C] float32 on the
    GPU.  C and O are positive multiples of 4, C at most max_channels() and O at most three times that."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(wq, torch.Tensor) or wq.dim() != 2:
        raise ValueError("x must be [N, C] and wq [O, C]")
    (N, C), O = x.shape, wq.shape[0]
    if C % 4 or O % 4 or C == 0 or O == 0:
        raise ValueError("C and O must be positive multiples of 4, got C = %d, O = %d" % (C, O))
    _check_float("x", x, (N, C))
    _check_float("s", s, (N, C))
    _check_float("wc", wc, (C, C))
    _check_float("wq", wq, (O, C))
    for name, v in (("bc", bc), ("lnc_w", lnc_w), ("lnc_b", lnc_b), ("ln1_w", ln1_w), ("ln1_b", ln1_b)):
        _check_float(name, v, (C,))
    _check_float("bq", bq, (O,))
    limit = max_channels()
    if C > limit or O > 3 * limit:
        raise ValueError("C = %d, O = %d: the fused kernels hold C up to %d and O up to %d" % (C, O, limit, 3 * limit))
    return ConvTailNormQkvFunction.apply(x, s, wc, bc, lnc_w, lnc_b, float(lnc_eps), ln1_w, ln1_b, float(ln1_eps), wq, bq)
