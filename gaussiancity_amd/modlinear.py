"""The grouped modulated linear layer of the generator's attribute head over libgcm_hip.so.

  modulated_linear(x [N, I], weight [O, I], alpha [G, I], beta [G, O], bias [O], group int32 [N], negative_slope)
        y[r] = leaky_relu((x[r] * alpha[group[r]]) @ weight.T + beta[group[r]] + bias); rows of group -1 give y = 0.
        alpha, beta, bias and group may each be None; gradients for x, weight, alpha, beta and bias, deterministic.
  groups_from_masks(masks, n)     int32 [n]: the largest g whose boolean mask has the row set, -1 where none has
  head_out(f, weight, bias, group, kind, factor)     the head's last linear layer and output transform, inference only
  head_chain(x, onehots, w1, b1, w_ma, w2, alpha, beta, bias2, group, w_out, b_out, kind, factor, negative_slope)
        the whole head for one output key in one launch, inference only: neither hidden activation reaches memory
  head_attrs(keys, group=None)                    {kind: [N, C]} for keys = {kind: (h, weight, bias or None, factor)}: the
        output layers and transforms of up to four keys in one launch, with gradients for every h, weight and bias
  head_points14(keys, xyz, scales, group=None)    the same, written as the rasterizer's [N, 14] record (helpers.
        get_gaussian_points on those values, xyz and scales untouched); the backward takes the record's gradient as it is

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation is in
the HIP library, float32 throughout, and nothing here waits for the device.
"""
import torch

from . import _native_m as M
from ._loader import current_stream as _stream
from ._loader import dense as _dense
from ._loader import fresh as _fresh

KINDS = tuple(M.KINDS)

_STATS = {"forward_calls": 0, "backward_calls": 0, "groups_from_masks_calls": 0, "head_out_calls": 0}
_CHAIN_STATS = {"head_chain_calls": 0}  # beside stats(), whose keys callers compare as a set
_HEAD_TRAIN_STATS = {"forward_calls": 0, "backward_calls": 0, "pre_stored": 0, "dh_outputs": 0, "dw_outputs": 0, "db_outputs": 0}


def stats():
    """Counters of this process: calls of each entry point of the library."""
    return dict(_STATS)


def chain_stats():
    """Counters of this process: calls of head_chain."""
    return dict(_CHAIN_STATS)


def head_train_stats():
    """Counters of this process: calls of gcm_head_train_forward and gcm_head_train_backward (head_attrs and head_points14
    together), forwards that stored `pre` for a backward, and the gradient tensors the backwards allocated -- an input that
    asks for no gradient gets none."""
    return dict(_HEAD_TRAIN_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0
    for k in _CHAIN_STATS:
        _CHAIN_STATS[k] = 0
    for k in _HEAD_TRAIN_STATS:
        _HEAD_TRAIN_STATS[k] = 0


def dtypes():
    """The element types the library's kernels run: (torch.float32,).  Loads the library."""
    M.lib()
    return (torch.float32,)


def _rows(t):
    """t [rows, width] as the library wants a row-strided operand: unit stride along the row, a row stride that is a
    positive multiple of 4 elements and at least the width, 16-byte aligned; a fresh dense copy otherwise."""
    if t.shape[0] == 0:  # no rows: whatever strides the empty tensor carries (numpy's are 0), the library gets dense ones
        return t.new_empty(t.shape)
    ok = t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= max(t.shape[1], 1) and t.data_ptr() % 16 == 0
    return t if ok else _fresh(t)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _grad32(dy):
    """An incoming gradient as the library reads it: float32, row-strided."""
    return _rows(dy if dy.dtype == torch.float32 else dy.float())


def _workspace(nbytes, device):
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def _check_float(name, t, shape, op="the modulated linear layer", optional=False):
    """t is a float32 tensor of `shape`, on the GPU.  op names the operator in the device message; None leaves the device
    to the caller (the operators that report it after every other check).  optional: None passes."""
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError("%s must be a float32 tensor (float16 is not supported)" % name)
    if op is not None and not t.is_cuda:
        raise TypeError("%s runs on the GPU; %s must be a CUDA tensor" % (op, name))
    if tuple(t.shape) != shape:
        raise ValueError("%s must be %r, got %r" % (name, shape, tuple(t.shape)))


class ModulatedLinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, alpha, beta, bias, group, slope, G):
        x, weight = _rows(x), _rows(weight)
        alpha, beta, bias = (None if t is None else _dense(t) for t in (alpha, beta, bias))
        N, I = x.shape
        O = weight.shape[0]
        y = x.new_empty((N, O))
        with torch.cuda.device(x.device):
            M.check(M.lib().gcm_modlinear_forward(x.data_ptr(), x.stride(0), weight.data_ptr(), weight.stride(0), _ptr(alpha),
                                                  _ptr(beta), _ptr(bias), _ptr(group), N, I, O, G, slope, y.data_ptr(),
                                                  y.stride(0), _stream()), "gcm_modlinear_forward")
        _STATS["forward_calls"] += 1
        ctx.save_for_backward(x, y, weight, alpha, group)
        ctx.meta = (slope, G, beta is not None, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, alpha, group = ctx.saved_tensors
        slope, G, has_beta, has_bias = ctx.meta
        N, I = x.shape
        O = weight.shape[0]
        dy = _grad32(dy)
        need = ctx.needs_input_grad
        dx = x.new_empty((N, I)) if need[0] else None
        dw = x.new_empty((O, I)) if need[1] else None
        dalpha = x.new_empty((G, I)) if alpha is not None and need[2] else None
        dbeta = x.new_empty((G, O)) if has_beta and need[3] else None
        dbias = x.new_empty((O,)) if has_bias and need[4] else None
        L = M.lib()
        ws_bytes = L.gcm_modlinear_backward_workspace_bytes(N, I, O, G)
        ws = _workspace(ws_bytes, x.device)
        with torch.cuda.device(x.device):
            M.check(L.gcm_modlinear_backward(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), dy.data_ptr(), dy.stride(0),
                                             weight.data_ptr(), weight.stride(0), _ptr(alpha), _ptr(group), N, I, O, G, slope,
                                             _ptr(dx), I, _ptr(dw), _ptr(dalpha), _ptr(dbeta), _ptr(dbias), ws.data_ptr(),
                                             ws_bytes, _stream()), "gcm_modlinear_backward")
        _STATS["backward_calls"] += 1
        return dx, dw, dalpha, dbeta, dbias, None, None, None


def _check_group(group, n):
    if group is None:
        return None
    if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or not group.is_cuda:
        raise TypeError("group must be an int32 CUDA tensor")
    if tuple(group.shape) != (n,):
        raise ValueError("group must be [%d], got %r" % (n, tuple(group.shape)))
    return group.contiguous()


def modulated_linear(x, weight, alpha=None, beta=None, bias=None, group=None, negative_slope=1.0):
    """leaky_relu((x * alpha[group]) @ weight.T + beta[group] + bias, negative_slope) for x [N, I], weight [O, I], alpha
    [G, I], beta [G, O], bias [O] float32 on the GPU and group int32 [N] with values in -1 .. G-1; I and O multiples of 4.
    A row of group -1 gives zeros and receives a zero gradient.  None for alpha / beta / bias / group means ones /
    zeros / zeros / every row in group 0; negative_slope 1 means no activation."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError("x must be [N, I] and weight [O, I]")
    (N, I), O = x.shape, weight.shape[0]
    if I % 4 or O % 4 or I == 0 or O == 0:
        raise ValueError("I and O must be positive multiples of 4, got I = %d, O = %d" % (I, O))
    G = alpha.shape[0] if isinstance(alpha, torch.Tensor) and alpha.dim() == 2 else (
        beta.shape[0] if isinstance(beta, torch.Tensor) and beta.dim() == 2 else 1)
    _check_float("x", x, (N, I))
    _check_float("weight", weight, (O, I))
    _check_float("alpha", alpha, (G, I), optional=True)
    _check_float("beta", beta, (G, O), optional=True)
    _check_float("bias", bias, (O,), optional=True)
    if G < 1:
        raise ValueError("alpha and beta need at least one group")
    slope = float(negative_slope)
    if not slope > 0.0:
        raise ValueError("negative_slope must be > 0 (got %r): the backward reads the sign of the stored output" % slope)
    return ModulatedLinearFunction.apply(x, weight, alpha, beta, bias, _check_group(group, N), slope, G)


def groups_from_masks(masks, n):
    """int32 [n] on the masks' device: for every row the largest g with masks[g][row] set (upstream's later assignment
    wins where masks overlap), -1 where no mask is set.  masks: a sequence of boolean CUDA tensors of n elements each.
    One launch whatever len(masks) is; the table of pointers is one host-to-device copy from pinned memory."""
    masks = [m.reshape(-1) if m.is_contiguous() else m.contiguous().reshape(-1) for m in masks]
    if not masks:
        raise ValueError("groups_from_masks needs at least one mask")
    for m in masks:
        if m.dtype != torch.bool or not m.is_cuda or m.numel() != n:
            raise TypeError("every mask must be a boolean CUDA tensor of %d elements" % n)
    dev = masks[0].device
    table = torch.tensor([m.data_ptr() for m in masks], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    group = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        M.check(M.lib().gcm_groups_from_masks(table.data_ptr(), len(masks), n, group.data_ptr(), _stream()),
                "gcm_groups_from_masks")
    _STATS["groups_from_masks_calls"] += 1
    return group


def head_out(f, weight, bias, group, kind, factor):
    """The head's output for one attribute, inference only (no autograd): transform(f @ weight.T + bias) for f [N, I],
    weight [C, I] (C = 1 or 3), bias [C] or None, kind in KINDS; rows of group -1 are zeros.  Returns [N, C]."""
    if kind not in M.KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    if not isinstance(f, torch.Tensor) or f.dim() != 2 or not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError("f must be [N, I] and weight [C, I]")
    (N, I), Cn = f.shape, weight.shape[0]
    if I % 4 or I == 0 or Cn not in (1, 3):
        raise ValueError("I must be a positive multiple of 4 and C 1 or 3, got I = %d, C = %d" % (I, Cn))
    _check_float("f", f, (N, I))
    _check_float("weight", weight, (Cn, I))
    _check_float("bias", bias, (Cn,), optional=True)
    group = _check_group(group, N)
    f, weight = _rows(f.detach()), _dense(weight.detach())
    bias = None if bias is None else _dense(bias.detach())
    out = f.new_empty((N, Cn))
    with torch.cuda.device(f.device):
        M.check(M.lib().gcm_head_out(f.data_ptr(), f.stride(0), weight.data_ptr(), _ptr(bias), _ptr(group), N, I, Cn,
                                     M.KINDS[kind], float(factor), out.data_ptr(), _stream()), "gcm_head_out")
    _STATS["head_out_calls"] += 1
    return out


def head_chain_limits():
    """(largest I, largest H) head_chain runs in this build.  Loads the library."""
    L = M.lib()
    return L.gcm_head_chain_max_in(), L.gcm_head_chain_max_hidden()


def head_chain(x, onehots, w1, b1, w_ma, w2, alpha, beta, bias2, group, w_out, b_out, kind, factor, negative_slope):
    """The attribute head for one output key in ONE launch, inference only (no autograd):
        f = leaky(x @ w1.T + onehots @ w_ma.T + b1);  h = leaky((f * alpha[group]) @ w2.T + beta[group] + bias2);
        transform(h @ w_out.T + b_out)
    for x [N, I], onehots [N, K] (any values), w1 [H, I], b1 [H], w_ma [H, K], w2 [H, H], alpha and beta [G, H] or None,
    bias2 [H] or None, group int32 [N] or None, w_out [C, H] (C = 1 or 3), b_out [C] or None, kind in KINDS.  I and H are
    multiples of 4 within head_chain_limits(), K is 1 .. 32; rows of group -1 are zeros.  Returns [N, C]."""
    if kind not in M.KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    for name, t in (("x", x), ("onehots", onehots), ("w1", w1), ("w_ma", w_ma), ("w2", w2), ("w_out", w_out)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError("x must be [N, I], onehots [N, K], w1 [H, I], w_ma [H, K], w2 [H, H] and w_out [C, H]; %s is not "
                             "a matrix" % name)
    (N, I), K, H, Cn = x.shape, onehots.shape[1], w1.shape[0], w_out.shape[0]
    if I % 4 or H % 4 or I == 0 or H == 0 or Cn not in (1, 3) or not 1 <= K <= 32:
        raise ValueError("I and H must be positive multiples of 4, K in 1..32 and C 1 or 3, got I = %d, H = %d, K = %d, C = %d"
                         % (I, H, K, Cn))
    G = alpha.shape[0] if isinstance(alpha, torch.Tensor) and alpha.dim() == 2 else (
        beta.shape[0] if isinstance(beta, torch.Tensor) and beta.dim() == 2 else 1)
    op = "the chained head"
    _check_float("x", x, (N, I), op)
    _check_float("onehots", onehots, (N, K), op)
    _check_float("w1", w1, (H, I), op)
    _check_float("b1", b1, (H,), op)
    _check_float("w_ma", w_ma, (H, K), op)
    _check_float("w2", w2, (H, H), op)
    _check_float("alpha", alpha, (G, H), op, optional=True)
    _check_float("beta", beta, (G, H), op, optional=True)
    _check_float("bias2", bias2, (H,), op, optional=True)
    _check_float("w_out", w_out, (Cn, H), op)
    _check_float("b_out", b_out, (Cn,), op, optional=True)
    if G < 1:
        raise ValueError("alpha and beta need at least one group")
    max_in, max_hidden = head_chain_limits()
    if I > max_in or H > max_hidden:
        raise ValueError("the chained head runs I <= %d and H <= %d, got I = %d, H = %d" % (max_in, max_hidden, I, H))
    slope = float(negative_slope)
    if not slope > 0.0:
        raise ValueError("negative_slope must be > 0, got %r" % slope)
    group = _check_group(group, N)
    dense = lambda t: None if t is None else _dense(t.detach())  # noqa: E731
    x, w1, w2 = _rows(x.detach()), _rows(w1.detach()), _rows(w2.detach())
    onehots = onehots.detach()
    if N and (onehots.stride(1) != 1 or onehots.stride(0) < K):
        onehots = onehots.contiguous()
    b1, w_ma, alpha, beta, bias2, w_out, b_out = (dense(t) for t in (b1, w_ma, alpha, beta, bias2, w_out, b_out))
    out = x.new_empty((N, Cn))
    with torch.cuda.device(x.device):
        M.check(M.lib().gcm_head_chain(x.data_ptr(), x.stride(0), onehots.data_ptr(), onehots.stride(0) if N else K,
                                       w1.data_ptr(), w1.stride(0), b1.data_ptr(), w_ma.data_ptr(), w2.data_ptr(), w2.stride(0),
                                       _ptr(alpha), _ptr(beta), _ptr(bias2), _ptr(group), w_out.data_ptr(), _ptr(b_out), N, I, K,
                                       H, G, Cn, M.KINDS[kind], float(factor), slope, out.data_ptr(), _stream()),
                "gcm_head_chain")
    _CHAIN_STATS["head_chain_calls"] += 1
    return out


# ---- the head's output layers in a training step -------------------------------------------------
def head_train_limit():
    """The largest hidden width head_attrs / head_points14 run in this build.  Loads the library."""
    return M.lib().gcm_head_train_max_in()


def _key_array(kinds, factors, hs, ws, bs):
    keys = (M.HeadKey * len(kinds))()
    for key, kind, factor, h, w, b in zip(keys, kinds, factors, hs, ws, bs):
        key.kind, key.factor, key.h, key.h_stride, key.w, key.b = M.KINDS[kind], factor, h.data_ptr(), h.stride(0), w.data_ptr(), _ptr(b)
    return keys


class HeadTrainFunction(torch.autograd.Function):
    """flat = (h, weight, bias) per key, in the order of kinds.  packed: the result is the [N, 14] record (one tensor),
    otherwise one [N, C] tensor per key."""

    @staticmethod
    def forward(ctx, kinds, factors, group, xyz, scales, packed, *flat):
        hs = [_rows(t) for t in flat[0::3]]
        ws = [_dense(t) for t in flat[1::3]]
        bs = [None if t is None else _dense(t) for t in flat[2::3]]
        N, I = hs[0].shape
        keys = _key_array(kinds, factors, hs, ws, bs)
        grad = any(ctx.needs_input_grad)
        L = M.lib()
        pre = hs[0].new_empty((N, L.gcm_head_train_pre_floats())) if grad else None
        if packed:
            outs = (hs[0].new_empty((N, 14)),)
        else:
            outs = tuple(hs[0].new_empty((N, w.shape[0])) for w in ws)
            for key, out in zip(keys, outs):
                key.out, key.out_stride = out.data_ptr(), out.shape[1]
        with torch.cuda.device(hs[0].device):
            M.check(L.gcm_head_train_forward(keys, len(kinds), _ptr(group), N, I, _ptr(pre), _ptr(xyz),
                                             xyz.stride(0) if packed and N else 3, _ptr(scales),
                                             scales.stride(0) if packed and N else 3, outs[0].data_ptr() if packed else None,
                                             _stream()), "gcm_head_train_forward")
        _HEAD_TRAIN_STATS["forward_calls"] += 1
        if grad:
            _HEAD_TRAIN_STATS["pre_stored"] += 1
            ctx.save_for_backward(pre, group, scales, *hs, *ws)
            ctx.meta = (kinds, factors, packed, [b is not None for b in bs])
        return outs[0] if packed else outs

    @staticmethod
    def backward(ctx, *douts):
        kinds, factors, packed, has_b = ctx.meta
        pre, group, scales = ctx.saved_tensors[:3]
        n = len(kinds)
        hs, ws = ctx.saved_tensors[3:3 + n], ctx.saved_tensors[3 + n:]
        N, I = hs[0].shape
        keys = _key_array(kinds, factors, hs, ws, [None] * n)
        need = ctx.needs_input_grad[6:]
        if packed:
            dp = douts[0] if douts[0].dtype == torch.float32 else douts[0].float()
            if N and (dp.stride(1) != 1 or dp.stride(0) < 14):
                dp = dp.contiguous()
        else:
            dp, held = None, []
            for key, w, d in zip(keys, ws, douts):
                d = d if d.dtype == torch.float32 else d.float()
                if N and (d.stride(1) != 1 or d.stride(0) < w.shape[0]):
                    d = d.contiguous()
                held.append(d)
                key.dout, key.dout_stride = d.data_ptr(), d.stride(0) if N else w.shape[0]
        grads = []
        for k, (key, h, w) in enumerate(zip(keys, hs, ws)):
            dh = h.new_empty((N, I)) if need[3 * k] else None
            dw = h.new_empty(tuple(w.shape)) if need[3 * k + 1] else None
            db = h.new_empty((w.shape[0],)) if has_b[k] and need[3 * k + 2] else None
            key.dh, key.dh_stride, key.dw, key.db = _ptr(dh), I, _ptr(dw), _ptr(db)
            for name, t in (("dh_outputs", dh), ("dw_outputs", dw), ("db_outputs", db)):
                _HEAD_TRAIN_STATS[name] += t is not None
            grads += [dh, dw, db]
        L = M.lib()
        ws_bytes = L.gcm_head_train_workspace_bytes(N, I, n)
        work = _workspace(ws_bytes, hs[0].device)
        with torch.cuda.device(hs[0].device):
            M.check(L.gcm_head_train_backward(keys, n, _ptr(group), N, I, pre.data_ptr(), _ptr(scales),
                                              scales.stride(0) if scales is not None and N else 3, _ptr(dp),
                                              dp.stride(0) if packed and N else 14, work.data_ptr(), ws_bytes, _stream()),
                    "gcm_head_train_backward")
        _HEAD_TRAIN_STATS["backward_calls"] += 1
        return (None, None, None, None, None, None, *grads)


def _check_head_keys(keys):
    """keys as head_attrs / head_points14 take them -> (kinds, factors, flat (h, weight, bias) per key, N)."""
    if not hasattr(keys, "items") or not 1 <= len(keys) <= 4:
        raise ValueError("keys must map one to four of %s to (h, weight, bias or None, factor)" % ", ".join(KINDS))
    kinds, factors, flat, shape = [], [], [], None
    limit = head_train_limit()
    for kind, entry in keys.items():
        if kind not in M.KINDS:
            raise ValueError("kind must be one of %s, got %r" % (", ".join(KINDS), kind))
        h, w, b, factor = entry
        if not isinstance(h, torch.Tensor) or h.dim() != 2 or not isinstance(w, torch.Tensor) or w.dim() != 2:
            raise ValueError("%s: h must be [N, I] and weight [C, I]" % kind)
        shape = tuple(h.shape) if shape is None else shape
        (N, I), Cn = shape, 1 if kind == "opacity" else 3
        if I % 4 or I == 0 or I > limit:
            raise ValueError("I must be a positive multiple of 4, at most %d, got %d" % (limit, I))
        op = "the head's output layers"
        _check_float(kind + ": h", h, (N, I), op)
        _check_float(kind + ": weight", w, (Cn, I), op)
        _check_float(kind + ": bias", b, (Cn,), op, optional=True)
        kinds.append(kind)
        factors.append(float(factor))
        flat += [h, w, b]
    return tuple(kinds), tuple(factors), flat, shape[0]


def head_attrs(keys, group=None):
    """The head's output layers for up to four attributes in ONE launch, with gradients: keys maps kind (of KINDS, each at
    most once, any order) to (h [N, I], weight [C, I], bias [C] or None, factor), C = 1 for opacity and 3 otherwise, all
    float32 on the GPU with the same N and I (a multiple of 4 within head_train_limit()).  Returns {kind: [N, C]} in the
    keys' order: transform(h @ weight.T + bias) with head_out's bits, exact zeros for a row whose group is negative.
    Every h, weight and bias that requires a gradient gets one; two keys may pass the same h."""
    kinds, factors, flat, N = _check_head_keys(keys)
    outs = HeadTrainFunction.apply(kinds, factors, _check_group(group, N), None, None, False, *flat)
    return dict(zip(kinds, outs))


def head_points14(keys, xyz, scales, group=None):
    """head_attrs written as the rasterizer's record [N, 14]: columns 0-2 xyz + attrs.xyz, 3 opacity (1 without the key), 4-6
    scales * attrs.scale, 7-10 (1, 0, 0, 0), 11-13 rgb -- helpers.get_gaussian_points on head_attrs' values, except that xyz
    and scales [N, >= 3] are read and left as they are.  keys needs "rgb"; xyz and scales are data and must not require a
    gradient.  The backward reads the [N, >= 14] gradient of the record as the rasterizer's node returns it."""
    kinds, factors, flat, N = _check_head_keys(keys)
    if "rgb" not in kinds:
        raise ValueError("head_points14 needs the rgb key")
    for name, t in (("xyz", xyz), ("scales", scales)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != N or t.shape[1] < 3:
            raise ValueError("%s must be [%d, >= 3]" % (name, N))
        if t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError("%s must be a float32 CUDA tensor" % name)
        if t.requires_grad:
            raise ValueError("%s is data here: it gets no gradient and must not require one" % name)
    dense = lambda t: t if t.shape[0] == 0 or t.stride(1) == 1 else t.contiguous()  # noqa: E731
    return HeadTrainFunction.apply(kinds, factors, _check_group(group, N), dense(xyz), dense(scales), True, *flat)
