"""Variable-length packed-QKV attention of the PTv3 point backbone over libgca_hip.so.

  varlen_qkvpacked(qkv [total, 3, H, d] fp16, cu_seqlens int32 [S + 1], max_seqlen, softmax_scale) -> [total, H, d]
  varlen_attention(qkv [total, 3, H, d] fp16 or fp32, ...)      the same operator for every dtype in dtypes(), result in
                                                                qkv.dtype: float32 never passes through binary16

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation
is in the HIP library, and nothing here waits for the device or reads cu_seqlens on the host.  The flash_attn
module at the repository root is the drop-in that models/pt_v3.py imports.
"""

import torch

from . import _native_a as A
from ._loader import current_stream as _stream
from ._loader import fresh as _fresh

SUPPORTED_HEAD_DIMS = A.HEAD_DIMS


def dtypes():
    """The element types the library's kernels run (gca_dtypes), in enum order: (torch.float16, torch.float32)."""
    bits = A.lib().gca_dtypes()
    return tuple(getattr(torch, name) for name, code in A.DTYPES.items() if bits >> code & 1)


def _kernel_ready(t):
    """Unit stride along the last dimension, every other stride a positive multiple of one 16-byte piece (8 float16, 4
    float32 elements), 16-byte aligned: what include/gca.h asks of a strided operand of t's dtype."""
    piece = 16 // t.element_size()
    return (t.stride(-1) == 1 and all(s > 0 and s % piece == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0)


def _dtype_code(dtype):
    return A.DTYPES[str(dtype).split(".")[-1]]


class VarlenQKVPackedFunction(torch.autograd.Function):
    """One function for every element type: the `_t` entry points with qkv.dtype's code (GCA_F16 through them is the
    untyped entry points, launch for launch)."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, softmax_scale):
        x = qkv if _kernel_ready(qkv) else _fresh(qkv)
        cu = cu_seqlens.contiguous()
        total, _, heads, d = x.shape
        nseg = cu.shape[0] - 1
        out = x.new_empty((total, heads, d))
        lse = torch.empty((heads, total), dtype=torch.float32, device=x.device)
        if total:
            with torch.cuda.device(x.device):
                A.check(A.lib().gca_varlen_forward_t(_dtype_code(x.dtype), x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                                                     cu.data_ptr(), nseg, total, heads, d, max_seqlen, softmax_scale,
                                                     out.data_ptr(), lse.data_ptr(), _stream()), "gca_varlen_forward_t")
        ctx.save_for_backward(x, out, lse, cu)
        ctx.meta = (max_seqlen, softmax_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, lse, cu = ctx.saved_tensors
        max_seqlen, softmax_scale = ctx.meta
        total, _, heads, d = x.shape
        nseg = cu.shape[0] - 1
        dy = dout if dout.dtype == x.dtype else dout.to(x.dtype)
        if not _kernel_ready(dy):
            dy = _fresh(dy)
        dqkv = x.new_empty((total, 3, heads, d))
        if total:
            L = A.lib()
            ws_bytes = L.gca_backward_workspace_bytes(total, heads)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
            with torch.cuda.device(x.device):
                A.check(L.gca_varlen_backward_t(_dtype_code(x.dtype), x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                                                out.data_ptr(), dy.data_ptr(), dy.stride(0), dy.stride(1), lse.data_ptr(),
                                                cu.data_ptr(), nseg, total, heads, d, max_seqlen, softmax_scale,
                                                dqkv.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "gca_varlen_backward_t")
        return dqkv, None, None, None


def _checked(qkv, cu_seqlens, max_seqlen, softmax_scale, dtype_error):
    """The argument checks of both public functions; `dtype_error` is the message for a qkv.dtype the caller refuses, or
    None.  Returns (max_seqlen, scale)."""
    if not isinstance(qkv, torch.Tensor) or not isinstance(cu_seqlens, torch.Tensor):
        raise TypeError("qkv and cu_seqlens must be tensors")
    if dtype_error is not None:
        raise TypeError(dtype_error)
    if cu_seqlens.dtype != torch.int32:
        raise TypeError("cu_seqlens must be int32 (got %s)" % cu_seqlens.dtype)
    if qkv.dim() != 4 or qkv.shape[1] != 3:
        raise ValueError("qkv must be [total, 3, heads, head_dim], got %r" % (tuple(qkv.shape),))
    if cu_seqlens.dim() != 1 or cu_seqlens.numel() < 1:
        raise ValueError("cu_seqlens must be 1-D with at least one entry, got %r" % (tuple(cu_seqlens.shape),))
    if qkv.shape[3] not in SUPPORTED_HEAD_DIMS:
        raise ValueError("head_dim %d is not supported; supported head dimensions: %s"
                         % (qkv.shape[3], ", ".join(str(d) for d in SUPPORTED_HEAD_DIMS)))
    if qkv.shape[2] < 1:
        raise ValueError("qkv needs at least one head, got %r" % (tuple(qkv.shape),))
    max_seqlen = int(max_seqlen)
    if max_seqlen < 0:
        raise ValueError("max_seqlen must not be negative (got %d)" % max_seqlen)
    if not qkv.is_cuda or not cu_seqlens.is_cuda:
        raise TypeError("attention runs on the GPU; qkv and cu_seqlens must be CUDA tensors")
    scale = float(qkv.shape[3]) ** -0.5 if softmax_scale is None else float(softmax_scale)
    return max_seqlen, scale


def varlen_qkvpacked(qkv, cu_seqlens, max_seqlen, softmax_scale=None):
    """softmax(softmax_scale * Q K^T) V per segment and head, not causal.  qkv [total, 3, H, d] float16 on the GPU
    (d in SUPPORTED_HEAD_DIMS), cu_seqlens int32 [S + 1]; returns [total, H, d] float16.  softmax_scale None means
    d ** -0.5.  Rows that no segment covers, and rows of a segment beyond its first max_seqlen, come back as zeros."""
    bad = isinstance(qkv, torch.Tensor) and qkv.dtype != torch.float16
    max_seqlen, scale = _checked(qkv, cu_seqlens, max_seqlen, softmax_scale,
                                 "qkv must be float16 (got %s); bfloat16 is not supported" % qkv.dtype if bad else None)
    return VarlenQKVPackedFunction.apply(qkv, cu_seqlens, max_seqlen, scale)


def varlen_attention(qkv, cu_seqlens, max_seqlen, softmax_scale=None):
    """varlen_qkvpacked for every element type of dtypes(): qkv float16 or float32, the result in qkv.dtype.  float32 is
    computed in fp32 throughout on the exact f32-input matrix instruction (include/gca.h has the rounding contract);
    float16 is varlen_qkvpacked, bit for bit."""
    bad = isinstance(qkv, torch.Tensor) and qkv.dtype not in (torch.float16, torch.float32)
    max_seqlen, scale = _checked(qkv, cu_seqlens, max_seqlen, softmax_scale,
                                 "qkv must be float16 or float32 (got %s); bfloat16 and float64 are not supported"
                                 % qkv.dtype if bad else None)
    return VarlenQKVPackedFunction.apply(qkv, cu_seqlens, max_seqlen, scale)
