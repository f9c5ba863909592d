"""The last stage of an inference frame on the device, over libgcv_hip.so (include/gcv.h K19): what
scripts/inference.py:255,264-272 does after the rasterizer --

    blurrer   = torchvision.transforms.GaussianBlur(kernel_size=3, sigma=(2, 2))
    road_mask = (torch.from_numpy(ins_map).cuda() == CLASSES[dataset]["ROAD"]).repeat(1, 3, 1, 1).float()
    fake_img  = blurrer(fake_img) * road_mask + fake_img * (1 - road_mask)

-- and, when asked, the uint8 conversion of :665-667, as ONE launch that reads the float image and the int16 instance
map points.visible_point_map leaves on the GPU.  No torchvision, no mask tensor, no host copy.

  gaussian_kernel2d(kernel_size, sigma)    the float32 [k,k] weight table, torchvision's recipe
  road_blur(img, ins_map, road_id, ...)    the finished frame: float in img's shape, or uint8 [H,W,3]
  frame_finish(img, ins_map, road_id, ...) both forms from one launch
  stats() / reset_stats()

CUDA float32 images run the HIP kernel; CPU tensors run a torch formulation of the same lines, so the function works
everywhere.  Inference only: there is no backward.
"""
import ctypes as C

import torch
import torch.nn.functional as F

_STATS = {"native_calls": 0, "fallback_calls": 0}
_KERNEL_SIZES = (3, 5, 7)  # radius 1..gcv_frame_finish_radius_max()
_weights = {}  # (kernel_size, sigma_x, sigma_y) -> (float32 [k,k] CPU tensor, ctypes float array of k*k)
_INT_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)


def stats():
    """Counters of this process: road_blur / frame_finish calls that ran the HIP kernel (`native_calls`) and calls that
    ran the torch formulation on CPU tensors (`fallback_calls`)."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _sigma_pair(sigma):
    if isinstance(sigma, (int, float)):
        sx = sy = float(sigma)
    else:
        s = tuple(float(v) for v in sigma)
        if len(s) != 2:
            raise ValueError("sigma must be a number or an (sigma_x, sigma_y) pair, got %r" % (sigma,))
        sx, sy = s
    if not (sx > 0.0 and sy > 0.0):
        raise ValueError("sigma must be positive, got %r" % (sigma,))
    return sx, sy


def _kernel1d(k, sigma):
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def _table(kernel_size, sigma):
    k = int(kernel_size)
    if k != kernel_size or k < 1 or k % 2 == 0:
        raise ValueError("kernel_size must be a positive odd integer, got %r" % (kernel_size,))
    sx, sy = _sigma_pair(sigma)
    e = _weights.get((k, sx, sy))
    if e is None:
        w = torch.mm(_kernel1d(k, sy)[:, None], _kernel1d(k, sx)[None, :]).contiguous()
        e = _weights[(k, sx, sy)] = (w, (C.c_float * (k * k))(*w.reshape(-1).tolist()))
    return e


def gaussian_kernel2d(kernel_size, sigma):
    """The [k,k] float32 weights of a Gaussian blur, computed in float32 by the recipe torchvision's GaussianBlur uses:
    x = linspace(-(k-1)/2, (k-1)/2, k); pdf = exp(-0.5 (x/sigma)^2); k1 = pdf / pdf.sum(); mm(k1_y[:,None], k1_x[None,:]).
    `sigma`: a float, or a pair (sigma_x, sigma_y).  (3, 2.0): centre 0.1308, corners 0.1019.  Built once per
    (kernel_size, sigma) and kept; a copy is returned."""
    return _table(kernel_size, sigma)[0].clone()


def _check(img, ins_map, kernel_size):
    if not isinstance(img, torch.Tensor) or img.dtype != torch.float32:
        raise TypeError("img must be a float32 tensor [3,H,W] or [B,3,H,W], got %s" %
                        (img.dtype if isinstance(img, torch.Tensor) else type(img).__name__))
    if img.dim() not in (3, 4) or img.shape[-3] != 3:
        raise ValueError("img must be [3,H,W] or [B,3,H,W], got %s" % (tuple(img.shape),))
    if torch.is_grad_enabled() and img.requires_grad:
        raise RuntimeError("road_blur finishes video frames: there is no backward through it (use no_grad)")
    if int(kernel_size) != kernel_size or int(kernel_size) not in _KERNEL_SIZES:
        raise ValueError("kernel_size must be 3, 5 or 7, got %r" % (kernel_size,))
    if not isinstance(ins_map, torch.Tensor):
        ins_map = torch.as_tensor(ins_map)
    if ins_map.dtype not in _INT_DTYPES:
        raise TypeError("ins_map must have an integer dtype, got %s" % ins_map.dtype)
    batched = img.dim() == 4
    b, h, w = (int(img.shape[0]) if batched else 1), int(img.shape[-2]), int(img.shape[-1])
    if tuple(ins_map.shape) not in ((h, w), (b, h, w)) or (ins_map.dim() == 3 and not batched):
        raise ValueError("ins_map must be [H,W] or [B,H,W] = %s for an image %s, got %s" %
                         ((b, h, w), tuple(img.shape), tuple(ins_map.shape)))
    r = int(kernel_size) // 2
    if b < 1 or h <= r or w <= r:  # torch: "Padding size should be less than the corresponding input dimension"
        raise ValueError("reflect padding of %d needs an image larger than that in both directions, got %dx%d (batch %d)" %
                         (r, h, w, b))
    return ins_map, batched, b, h, w


def _video_bytes(img4, bgr):
    """InferenceLoop.to_uint8_hwc per image of [B,3,H,W]."""
    u8 = ((img4.clamp(-1, 1) / 2 + 0.5) * 255).permute(0, 2, 3, 1).to(torch.uint8)
    return (u8.flip(-1) if bgr else u8).contiguous()


def _torch_finish(img4, map3, road_id, weights, flip_mask_lr, want_f32, want_u8, bgr):
    """The torch formulation (any device): reflect pad + depthwise conv2d + select."""
    k = int(weights.shape[0])
    w = weights.to(img4.device)[None, None].expand(3, 1, k, k)
    blurred = F.conv2d(F.pad(img4, (k // 2,) * 4, mode="reflect"), w, groups=3)
    road = (map3.flip(-1) if flip_mask_lr else map3) == int(road_id)
    out = torch.where(road[:, None], blurred, img4)
    return (out if want_f32 else None), (_video_bytes(out, bgr) if want_u8 else None)


def _native_finish(img4, map3, road_id, table, flip_mask_lr, want_f32, want_u8, bgr):
    from . import _native_v as V
    from ._loader import current_stream
    dev = img4.device
    b, _, h, w = (int(v) for v in img4.shape)
    if w > 1 and img4.stride(3) != 1:
        img4 = img4.contiguous()
    if map3.device != dev:
        map3 = map3.to(dev)
    map3 = map3.contiguous()
    out_f = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev) if want_f32 else None
    out_u = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    k = int(table[0].shape[0])
    with torch.cuda.device(dev):
        V.check(V.lib().gcv_frame_finish(
            img4.data_ptr(), img4.stride(0) if b > 1 else 0, img4.stride(1), img4.stride(2) if h > 1 else 0, b, h, w,
            map3.data_ptr(), h * w if map3.shape[0] > 1 else 0, int(road_id), int(bool(flip_mask_lr)), k // 2, table[1],
            None if out_f is None else out_f.data_ptr(), None if out_u is None else out_u.data_ptr(), int(bool(bgr)),
            current_stream()), "gcv_frame_finish")
    _STATS["native_calls"] += 1
    return out_f, out_u


def frame_finish(img, ins_map, road_id, kernel_size=3, sigma=2.0, flip_mask_lr=False, want_float=True, want_uint8=True,
                 bgr=False):
    """Both forms of the finished frame from one launch: (float image in img's shape or None, uint8 [H,W,3] /
    [B,H,W,3] or None).  Arguments as road_blur."""
    if not (want_float or want_uint8):
        raise ValueError("frame_finish: nothing to compute (want_float and want_uint8 are both False)")
    ins_map, batched, b, h, w = _check(img, ins_map, kernel_size)
    if not -32768 <= int(road_id) <= 32767:
        raise ValueError("road_id must be an int16 value, got %r" % (road_id,))
    table = _table(kernel_size, sigma)
    img4 = img.detach() if batched else img.detach()[None]
    map3 = ins_map if ins_map.dim() == 3 else ins_map[None]
    if map3.dtype != torch.int16:
        map3 = map3.to(torch.int16)
    if img4.is_cuda:
        out_f, out_u = _native_finish(img4, map3, road_id, table, flip_mask_lr, want_float, want_uint8, bgr)
    elif img4.device.type == "cpu":
        out_f, out_u = _torch_finish(img4, map3.to(img4.device), road_id, table[0], flip_mask_lr, want_float, want_uint8, bgr)
        _STATS["fallback_calls"] += 1
    else:
        raise TypeError("img must live on a GPU or on the CPU, got %s" % img4.device)
    if not batched:
        out_f, out_u = (None if out_f is None else out_f[0]), (None if out_u is None else out_u[0])
    return out_f, out_u


def road_blur(img, ins_map, road_id, kernel_size=3, sigma=2.0, flip_mask_lr=False, as_uint8=False, bgr=False):
    """scripts/inference.py:255,264-272: Gaussian-blurs the pixels that show a road, leaves every other pixel as it is.

    img: float32 [3,H,W] or [B,3,H,W], never written.  ins_map: [H,W] (one map for every image) or [B,H,W], an integer
    dtype (instance ids are int16 throughout this package: any other integer dtype is converted to int16 first), a
    tensor on img's device or anything torch.as_tensor takes; points.visible_point_map's second result as it is.
    A pixel (y, x) shows a road where ins_map[y, x] == road_id, or ins_map[y, W-1-x] with flip_mask_lr (an image the
    rasterizer wrapper flipped, a map that was not).  kernel_size 3, 5 or 7; sigma a float or (sigma_x, sigma_y).

    Returns the float image in img's shape -- road pixels the float32 stencil sum in row-major tap order over torch's
    reflect padding, all others bit for bit the input -- or, with as_uint8, the video frame uint8 [H,W,3] / [B,H,W,3] that
    InferenceLoop.to_uint8_hwc would make of it (bgr=True: channels reversed, the img[..., ::-1] cv2 wants, :666-667).

    A CUDA image is one gcv_frame_finish launch on the current stream with no host wait; its strides are passed through
    when the pixel stride is 1, otherwise a contiguous copy is taken.  A CPU image runs F.pad(reflect) + a depthwise
    F.conv2d + a select.  Other dtypes: TypeError.  H or W <= kernel_size // 2 (where torch refuses the padding):
    ValueError.  A tensor that requires grad under enabled grad: RuntimeError.

    Deliberate difference from upstream: GaussianBlur(sigma=(2, 2)) draws its sigma from the interval [2, 2] with the
    global CPU generator on every call -- always 2, but the generator advances.  road_blur takes the value and draws
    nothing, so code after it sees a generator state upstream's would not have."""
    out_f, out_u = frame_finish(img, ins_map, road_id, kernel_size, sigma, flip_mask_lr, want_float=not as_uint8,
                                want_uint8=bool(as_uint8), bgr=bgr)
    return out_u if as_uint8 else out_f
