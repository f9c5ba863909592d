"""The seams between the PTv3 stages over libgcm_hip.so (include/gcm.h): the chain
Linear -> BatchNorm1d -> GELU that Embedding.stem, SerializedPooling and SerializedUnpooling run between the stages, as one
operator.

  linear_bn_gelu(x [N, I], weight [O, I] or None, bias [O] or None, bn_weight [O], bn_bias [O], running_mean [O],
                 running_var [O], num_batches_tracked [], *, training, momentum, eps, act=True) -> [N, O]
        gelu(batch_norm(x @ weight.T + bias)).  weight=None is the chain without a product (I == O, bias must be None);
        act=False the chain without the GELU.  training=False reads the running statistics: one launch, nothing but the
        result reaches memory unless a gradient is needed.  training=True uses the batch's statistics (three launches) and
        updates the three buffers in place on the device, as BatchNorm1d does (the three may all be None: nothing is
        tracked then; a buffer that is not 16-byte aligned, such as a view into a flat buffer, is updated through an
        aligned temporary that the same stream copies back); it saves x, z, mean and rstd for the gradient, never u or the
        result.  Gradients for x, weight, bias, bn_weight and bn_bias, deterministic (no float atomics).
  max_channels()                  the largest I and O the kernels run
  stats() / reset_stats()

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation is in
the HIP library, float32 throughout, and nothing here waits for the device, forward or backward.
"""
import functools

import torch

from . import _native_m as M
from ._loader import current_stream as _stream
from ._loader import dense as _dense
from .modlinear import _check_float as _check_float_op
from .modlinear import _grad32, _ptr, _rows, _workspace

_check_float = functools.partial(_check_float_op, op=None)  # the device is checked after everything else

_STATS = {"forward_eval_calls": 0, "forward_train_calls": 0, "backward_calls": 0}


def stats():
    """Counters of this process: calls of the library's entry points."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def max_channels():
    """The largest I and O the library's kernels run.  Loads the library."""
    return int(M.lib().gcm_seam_max_channels())


def _check_cuda(name, t):
    if not t.is_cuda:
        raise TypeError("the fused stage seam runs on the GPU; %s must be a CUDA tensor" % name)


class LinearBnGeluFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn_weight, bn_bias, running_mean, running_var, tracked, training, momentum, eps, act):
        x = _rows(x)
        weight, bias = (None if t is None else _dense(t) for t in (weight, bias))
        bn_weight, bn_bias = _dense(bn_weight), _dense(bn_bias)
        # the running statistics as the library takes them (dense, 16-byte aligned): the caller's buffers wherever they
        # are that, else aligned temporaries, which a training step copies back into the buffers on the same stream
        stat_mean, stat_var = (None if t is None else _dense(t) for t in (running_mean, running_var))
        N, I = x.shape
        O = I if weight is None else weight.shape[0]
        need = any(ctx.needs_input_grad)
        y = x.new_empty((N, O))
        L = M.lib()
        z = mean = rstd = None
        with torch.cuda.device(x.device):
            if training:
                z = x.new_empty((N, O)) if weight is not None else None
                mean, rstd = x.new_empty((O,)), x.new_empty((O,))
                ws_bytes = L.gcm_seam_forward_workspace_bytes(N, O)
                ws = _workspace(ws_bytes, x.device)
                M.check(L.gcm_seam_forward_train(x.data_ptr(), x.stride(0), _ptr(weight), _ptr(bias), eps, momentum,
                                                 bn_weight.data_ptr(), bn_bias.data_ptr(), int(act), N, I, O, _ptr(z),
                                                 y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(),
                                                 _ptr(stat_mean), _ptr(stat_var), _ptr(tracked), ws.data_ptr(), ws_bytes,
                                                 _stream()), "gcm_seam_forward_train")
                for buffer, stat in ((running_mean, stat_mean), (running_var, stat_var)):
                    if stat is not buffer:
                        buffer.copy_(stat)
                _STATS["forward_train_calls"] += 1
            else:
                if need:  # a gradient in eval mode: the launch also leaves z and rstd
                    z = x.new_empty((N, O)) if weight is not None else None
                    rstd = x.new_empty((O,))
                    mean = stat_mean.clone()  # the buffer may be updated in place before the backward runs
                M.check(L.gcm_seam_forward_eval(x.data_ptr(), x.stride(0), _ptr(weight), _ptr(bias), stat_mean.data_ptr(),
                                                stat_var.data_ptr(), eps, bn_weight.data_ptr(), bn_bias.data_ptr(),
                                                int(act), N, I, O, y.data_ptr(), y.stride(0), _ptr(z), _ptr(rstd), _stream()),
                        "gcm_seam_forward_eval")
                _STATS["forward_eval_calls"] += 1
        if need:
            ctx.save_for_backward(x, z, mean, rstd, weight, bn_weight, bn_bias)
            ctx.seam = (bool(training), bool(act), bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z, mean, rstd, weight, bn_weight, bn_bias = ctx.saved_tensors
        training, act, has_bias = ctx.seam
        need = ctx.needs_input_grad
        g = _grad32(dy)
        N, I = x.shape
        O = bn_weight.shape[0]
        product = weight is not None
        dx = x.new_empty((N, I)) if need[0] else None
        dw = x.new_empty((O, I)) if product and need[1] else None
        db = x.new_empty((O,)) if product and has_bias and need[2] else None
        dg = x.new_empty((O,)) if need[3] else None
        dh = x.new_empty((O,)) if need[4] else None
        zz = z if product else x
        L = M.lib()
        ws_bytes = L.gcm_seam_backward_workspace_bytes(N, I, O)
        ws = _workspace(ws_bytes, x.device)
        with torch.cuda.device(x.device):
            M.check(L.gcm_seam_backward(x.data_ptr(), x.stride(0), zz.data_ptr(), zz.stride(0), mean.data_ptr(),
                                        rstd.data_ptr(), g.data_ptr(), g.stride(0), _ptr(weight), bn_weight.data_ptr(),
                                        bn_bias.data_ptr(), int(act), int(training), N, I, O, _ptr(dx),
                                        0 if dx is None else dx.stride(0), _ptr(dw), _ptr(db), _ptr(dg), _ptr(dh),
                                        ws.data_ptr(), ws_bytes, _stream()), "gcm_seam_backward")
        _STATS["backward_calls"] += 1
        return dx, dw, db, dg, dh, None, None, None, None, None, None, None


def linear_bn_gelu(x, weight, bias, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, *, training,
                   momentum, eps, act=True):
    """gelu(batch_norm(x @ weight.T + bias)) for x [N, I], weight [O, I] (None: no product, bias None too), bias [O] or
    None, bn_weight and bn_bias [O], all float32 on the GPU; running_mean and running_var [O] float32 and
    num_batches_tracked a 0-d int64 tensor, updated in place when training (all three None: nothing tracked, training
    only).  I and O are positive multiples of 4, at most max_channels(); training needs N >= 2 or N == 0."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("x must be [N, I]")
    N, I = x.shape
    if weight is None:
        if bias is not None:
            raise ValueError("bias needs weight: weight=None is the chain without a product")
        O = I
    else:
        if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
            raise ValueError("weight must be [O, I]")
        O = weight.shape[0]
    for name, width in (("I", I), ("O", O)):
        if width % 4 or width == 0:
            raise ValueError("%s must be a positive multiple of 4, got %s = %d" % (name, name, width))
        if width > max_channels():
            raise ValueError("%s = %d: the fused kernels hold %s up to %d" % (name, width, name, max_channels()))
    if not isinstance(momentum, (int, float)) or not 0.0 <= momentum <= 1.0:
        raise ValueError("momentum must be a number in 0..1, got %r" % (momentum,))
    if not isinstance(eps, (int, float)) or not eps >= 0.0 or eps == float("inf"):
        raise ValueError("eps must be finite and >= 0, got %r" % (eps,))
    if training and N == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %r" % (tuple(x.shape),))
    _check_float("x", x, (N, I))
    if weight is not None:
        _check_float("weight", weight, (O, I))
    if bias is not None:
        _check_float("bias", bias, (O,))
    _check_float("bn_weight", bn_weight, (O,))
    _check_float("bn_bias", bn_bias, (O,))
    buffers = (running_mean, running_var, num_batches_tracked)
    if any(b is None for b in buffers):
        if not all(b is None for b in buffers):
            raise ValueError("running_mean, running_var and num_batches_tracked come together, all or none")
        if not training:
            raise ValueError("eval mode reads running_mean and running_var")
    else:
        _check_float("running_mean", running_mean, (O,))
        _check_float("running_var", running_var, (O,))
        if not isinstance(num_batches_tracked, torch.Tensor) or num_batches_tracked.dtype != torch.int64 \
                or num_batches_tracked.numel() != 1:
            raise TypeError("num_batches_tracked must be an int64 tensor of one element")
        for name, b in (("running_mean", running_mean), ("running_var", running_var)):
            if not b.is_contiguous() or b.requires_grad:
                raise ValueError("%s must be a contiguous buffer that requires no gradient" % name)
    named = {"x": x, "weight": weight, "bias": bias, "bn_weight": bn_weight, "bn_bias": bn_bias,
             "running_mean": running_mean, "running_var": running_var, "num_batches_tracked": num_batches_tracked}
    for name, t in named.items():
        if t is not None:
            _check_cuda(name, t)
    return LinearBnGeluFunction.apply(x, weight, bias, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked,
                                      bool(training), float(momentum), float(eps), bool(act))
