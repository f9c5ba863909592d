"""The image-side losses of a training step over libgcv_hip.so (include/gcv.h K20-K22): what
core/train.py:227-295 runs as some forty small torch kernels per iteration --

    l1(a, b, mask=None)                              torch.nn.L1Loss()(a * mask, b * mask)            (train.py:285)
    gan_loss(pred, label, weight=None, real=True)    losses.gan.GANLoss.loss                          (losses/gan.py:55-97)
    label_map(seg, size, mask=None)                  Discriminator._smooth_interp(seg * mask, size)   (discriminator.py:177-189)
    GANLoss                                          a drop-in for losses.gan.GANLoss over gan_loss
    install(gan_module, discriminator_module) / uninstall(...)   rebind the two upstream functions
    stats() / reset_stats()

-- as two launches per loss forward (partial sums per workgroup, then a fold in a fixed order), one launch per backward
and one launch for the label map.  The sums are cut by the shape alone and use no atomics: two runs give the same bits.
A backward recomputes its terms from the saved inputs and reads the incoming gradient on the device; the forward writes
no gradient.  Nothing waits for the device.

CUDA float32 tensors run the kernels; their strides are passed through when the pixel stride is 1, otherwise one
contiguous copy is taken.  The torch formulation of upstream's lines (torch_l1, torch_gan_loss, torch_label_map) runs
instead for CPU tensors, other dtypes, autocast, more than max_classes() channels, a mask / label / weight that requires
grad or has another shape than [B, 1, H, W] / [B, C, h, w], and a label map larger than its source.
"""
import ctypes as C
import inspect

import torch
import torch.nn.functional as F

_STATS = {"native_calls": 0, "fallback_calls": 0}
_ORIGINAL_LOSS = "_gaussiancity_amd_image_loss_original_loss"
_ORIGINAL_INTERP = "_gaussiancity_amd_image_loss_original_smooth_interp"
_MAX_ELEMENTS = 2 ** 31 - 1
_S3, _S2 = C.c_int64 * 3, C.c_int64 * 2


def stats():
    """Counters of this process: l1 / gan_loss / label_map calls that ran the HIP kernels (`native_calls`) and calls that
    ran the torch formulation (`fallback_calls`)."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def max_classes():
    """The most channels gan_loss's label and label_map's seg may have on the kernel path (32)."""
    from . import _native_v as V
    return int(V.lib().gcv_image_loss_max_classes())


# ---- the torch formulations: upstream's lines, on any device and dtype ---------------------------------------------------
def torch_l1(a, b, mask=None):
    if mask is not None:
        a, b = a * mask, b * mask
    return F.l1_loss(a, b)


def torch_gan_loss(pred, label, weight=None, real=True):
    assert pred.size(1) == label.size(1) + 1
    pred, label = pred.clone(), label.clone()
    label[:, 0] = 0
    pred[:, 0] = 0
    logp = F.log_softmax(pred, dim=1)
    if real:
        per = (-label * logp[:, :-1]).sum(dim=1, keepdim=True)
    else:
        per = -logp[:, -1:]
    if weight is not None:
        per = per * weight
    return per.mean()


def torch_label_map(seg, size, mask=None):
    x = F.interpolate(seg if mask is None else seg * mask, size=size, mode="area")
    idx = torch.argmax(x, dim=1, keepdim=True)
    return torch.zeros_like(x).scatter_(1, idx, 1.0)


# ---- the kernel path -----------------------------------------------------------------------------------------------------
def _f32_cuda(*tensors):
    return all(t is None or (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32) for t in tensors)


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _unit(t):
    """t with pixel stride 1 (a contiguous copy where it has another)."""
    return t if t is None or t.shape[-1] == 1 or t.stride(-1) == 1 else t.contiguous()


def _s3(t):
    return _S3(t.stride(0), t.stride(1), t.stride(2))


def _s2(t):
    return None if t is None else _S2(t.stride(0), t.stride(2))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _partials(V, n, pixels, dev):
    k = int(V.lib().gcv_image_loss_partials(n, pixels))
    if k <= 0:
        V.check(-1, "gcv_image_loss_partials")
    return torch.empty(k, dtype=torch.float64, device=dev), k


def _l1_native_ok(a, b, mask):
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or not _f32_cuda(a, b, mask):
        return False
    if torch.is_autocast_enabled() or a.dim() != 4 or a.shape != b.shape or not 0 < a.numel() <= _MAX_ELEMENTS:
        return False
    if mask is not None and (tuple(mask.shape) != (a.shape[0], 1, a.shape[2], a.shape[3]) or _needs_grad(mask)):
        return False
    return a.device == b.device and (mask is None or mask.device == a.device)


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mask):
        from . import _native_v as V
        from ._loader import current_stream
        a, b, mask = _unit(a.detach()), _unit(b.detach()), _unit(None if mask is None else mask.detach())
        B, Ch, H, W = (int(v) for v in a.shape)
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            part, k = _partials(V, a.numel(), 0, a.device)
            V.check(V.lib().gcv_mean_abs_forward(a.data_ptr(), _s3(a), b.data_ptr(), _s3(b), _ptr(mask), _s2(mask), B, Ch, H, W,
                                           part.data_ptr(), k, loss.data_ptr(), current_stream()), "gcv_mean_abs_forward")
        ctx.save_for_backward(a, b, mask)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import _native_v as V
        from ._loader import current_stream
        a, b, mask = ctx.saved_tensors
        B, Ch, H, W = (int(v) for v in a.shape)
        g = g.to(torch.float32).contiguous()
        da = torch.empty(a.shape, dtype=torch.float32, device=a.device) if ctx.needs_input_grad[0] else None
        db = torch.empty(a.shape, dtype=torch.float32, device=a.device) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(a.device):
            V.check(V.lib().gcv_mean_abs_backward(a.data_ptr(), _s3(a), b.data_ptr(), _s3(b), _ptr(mask), _s2(mask), B, Ch, H, W,
                                            g.data_ptr(), _ptr(da), _ptr(db), current_stream()), "gcv_mean_abs_backward")
        return da, db, None


def l1(a, b, mask=None):
    """torch.nn.L1Loss()(a * mask, b * mask) (core/train.py:285), or L1Loss()(a, b) with mask None: a 0-d tensor.

    a, b: float32 [B, C, H, W] of one shape; mask: float32 [B, 1, H, W] of any values.  The term is
    t = fl(fl(a m) - fl(b m)), the loss sum |t| / (B C H W); da = g sign(t) m / count and db = -da, each only where that
    input requires a gradient (sign(0) = 0).  On the device: two launches forward, one backward (which recomputes t; the
    forward writes no gradient), inputs never written."""
    if _l1_native_ok(a, b, mask):
        _STATS["native_calls"] += 1
        return _L1.apply(a, b, mask)
    _STATS["fallback_calls"] += 1
    return torch_l1(a, b, mask)


def _gan_native_ok(pred, label, weight):
    if not (isinstance(pred, torch.Tensor) and isinstance(label, torch.Tensor)) or not _f32_cuda(pred, label):
        return False
    if weight is not None and not (isinstance(weight, torch.Tensor) and _f32_cuda(weight)):
        return False
    if torch.is_autocast_enabled() or pred.dim() != 4 or label.dim() != 4 or not 0 < pred.numel() <= _MAX_ELEMENTS:
        return False
    B, C1, h, w = pred.shape
    if tuple(label.shape) != (B, C1 - 1, h, w) or not 1 <= C1 - 1 <= max_classes() or _needs_grad(label, weight):
        return False
    if weight is not None and (tuple(weight.shape) != (B, 1, h, w) or weight.device != pred.device):
        return False
    return label.device == pred.device


class _Gan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, weight, real):
        from . import _native_v as V
        from ._loader import current_stream
        pred, label, weight = _unit(pred.detach()), _unit(label.detach()), _unit(None if weight is None else weight.detach())
        B, C1, h, w = (int(v) for v in pred.shape)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            part, k = _partials(V, B * h * w, 1, pred.device)
            V.check(V.lib().gcv_gan_loss_forward(pred.data_ptr(), _s3(pred), label.data_ptr(), _s3(label), _ptr(weight), _s2(weight),
                                                 B, C1 - 1, h, w, int(real), part.data_ptr(), k, loss.data_ptr(),
                                                 current_stream()), "gcv_gan_loss_forward")
        ctx.save_for_backward(pred, label, weight)
        ctx.real = int(real)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import _native_v as V
        from ._loader import current_stream
        pred, label, weight = ctx.saved_tensors
        B, C1, h, w = (int(v) for v in pred.shape)
        g = g.to(torch.float32).contiguous()
        dpred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            V.check(V.lib().gcv_gan_loss_backward(pred.data_ptr(), _s3(pred), label.data_ptr(), _s3(label), _ptr(weight), _s2(weight),
                                                  B, C1 - 1, h, w, ctx.real, g.data_ptr(), dpred.data_ptr(), current_stream()),
                    "gcv_gan_loss_backward")
        return dpred, None, None, None


def gan_loss(pred, label, weight=None, real=True):
    """The N+1-label GAN loss of losses/gan.py:55-97 as one operator: a 0-d tensor.

    pred: float32 [B, C+1, h, w]; label: float32 [B, C, h, w]; weight: None or float32 [B, 1, h, w].  Per pixel, with
    channel 0 of pred and of label counted as 0 and lse the log-sum-exp of the C+1 logits (the pixel's maximum is
    subtracted first): real=True -- upstream's (t_real=True, dis_update=True) and (True, False), the same arithmetic --
    is sum_{c<C} label_c (lse - pred_c), real=False -- (False, True) -- is lse - pred_C; the loss is the mean of
    weight * that over B h w.  The gradient goes to pred only and is exactly 0 in channel 0.  On the device: two launches
    forward, one backward (which recomputes the softmax; the forward writes no gradient)."""
    if _gan_native_ok(pred, label, weight):
        _STATS["native_calls"] += 1
        return _Gan.apply(pred, label, weight, bool(real))
    _STATS["fallback_calls"] += 1
    return torch_gan_loss(pred, label, weight, real)


def label_map(seg, size, mask=None):
    """Discriminator._smooth_interp(seg * mask, size) (models/discriminator.py:177-189, used at :219): area interpolation
    to size = (h, w), then a one-hot of the first maximal channel -- a new float32 [B, C, h, w] of zeros and ones.

    seg: float32 [B, C, H, W]; mask: None or [B, 1, H, W].  The kernel (one launch) compares the channels' window sums,
    each added in row-major order; all channels of a pixel share the divisor, so that is the comparison of the means
    wherever the sums are exact (one-hot maps times a binary mask), and a tie goes to the lowest channel: a window that is
    masked out entirely gives channel 0, which gan_loss ignores.  There is no gradient: a tensor that requires grad under
    enabled grad is refused (RuntimeError)."""
    if not isinstance(seg, torch.Tensor) or seg.dim() != 4:
        raise ValueError("seg must be a tensor [B, C, H, W]")
    if _needs_grad(seg, mask):
        raise RuntimeError("label_map makes a one-hot label: there is no backward through it (use no_grad or detach)")
    h, w = (int(v) for v in size)
    B, Ch, H, W = (int(v) for v in seg.shape)
    native = (_f32_cuda(seg, mask) and not torch.is_autocast_enabled() and 1 <= Ch <= max_classes() and 1 <= h <= H and 1 <= w <= W
              and 0 < seg.numel() <= _MAX_ELEMENTS
              and (mask is None or (tuple(mask.shape) == (B, 1, H, W) and mask.device == seg.device)))
    if not native:
        _STATS["fallback_calls"] += 1
        with torch.no_grad():
            return torch_label_map(seg, (h, w), mask)
    from . import _native_v as V
    from ._loader import current_stream
    seg, mask = _unit(seg.detach()), _unit(None if mask is None else mask.detach())
    out = torch.empty((B, Ch, h, w), dtype=torch.float32, device=seg.device)
    with torch.cuda.device(seg.device):
        V.check(V.lib().gcv_label_map(seg.data_ptr(), _s3(seg), _ptr(mask), _s2(mask), B, Ch, H, W, h, w, out.data_ptr(),
                                      current_stream()), "gcv_label_map")
    _STATS["native_calls"] += 1
    return out


# ---- drop-ins ------------------------------------------------------------------------------------------------------------
def _loss_method(self, input_x, t_real, weight=None, reduce_dim=True, dis_update=True):
    """GANLoss.loss over gan_loss, with upstream's assertions."""
    assert reduce_dim is True
    pred, label = input_x["pred"], input_x["label"]
    assert pred.size(1) == label.size(1) + 1
    if not dis_update:
        assert t_real, "GAN loss must be aiming for real."
    return gan_loss(pred, label, weight, real=bool(t_real))


class GANLoss(torch.nn.Module):
    """A drop-in for losses.gan.GANLoss: the same constructor and forward(input_x, t_real, weight=None, reduce_dim=True,
    dis_update=True) for a {"pred", "label"} dict or a list of them (a list element that is itself a list stands for its
    last entry; the list's losses are averaged), every loss through gan_loss."""

    def __init__(self, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.real_label, self.fake_label = target_real_label, target_fake_label
        self.real_label_tensor = self.fake_label_tensor = None

    loss = _loss_method

    def forward(self, input_x, t_real, weight=None, reduce_dim=True, dis_update=True):
        if not isinstance(input_x, list):
            return self.loss(input_x, t_real, weight, reduce_dim, dis_update)
        total = 0
        for item in input_x:
            one = self.loss(item[-1] if isinstance(item, list) else item, t_real, weight, reduce_dim, dis_update)
            total = total + one.reshape(1 if one.dim() == 0 else one.size(0), -1).mean(dim=1)
        return total / len(input_x)


def _smooth_interp(x, size):
    return label_map(x, size)


def install(gan_module=None, discriminator_module=None):
    """Rebind GANLoss.loss of the caller's imported losses.gan and Discriminator._smooth_interp of the caller's imported
    models.discriminator to gan_loss and label_map.  Either module may be None; idempotent; uninstall() puts the modules'
    own functions back, which are kept on the module meanwhile.

    Discriminator.__init__ stores self._smooth_interp in self.interpolator, so a Discriminator built BEFORE install keeps
    upstream's function (and one built after it keeps label_map after uninstall): install first, then build the model.
    Upstream calls the interpolator on seg_maps * masks, so the product stays a torch kernel on that path; label_map's own
    mask argument is for callers that have both tensors."""
    if gan_module is not None and getattr(gan_module, _ORIGINAL_LOSS, None) is None:
        max_classes()  # loads the library: a missing build fails here, not inside a training step
        setattr(gan_module, _ORIGINAL_LOSS, gan_module.GANLoss.loss)
        gan_module.GANLoss.loss = _loss_method
    if discriminator_module is not None and getattr(discriminator_module, _ORIGINAL_INTERP, None) is None:
        max_classes()
        setattr(discriminator_module, _ORIGINAL_INTERP, inspect.getattr_static(discriminator_module.Discriminator, "_smooth_interp"))  # the staticmethod object
        discriminator_module.Discriminator._smooth_interp = staticmethod(_smooth_interp)


def uninstall(gan_module=None, discriminator_module=None):
    if gan_module is not None and getattr(gan_module, _ORIGINAL_LOSS, None) is not None:
        gan_module.GANLoss.loss = getattr(gan_module, _ORIGINAL_LOSS)
        delattr(gan_module, _ORIGINAL_LOSS)
    if discriminator_module is not None and getattr(discriminator_module, _ORIGINAL_INTERP, None) is not None:
        discriminator_module.Discriminator._smooth_interp = getattr(discriminator_module, _ORIGINAL_INTERP)
        delattr(discriminator_module, _ORIGINAL_INTERP)
