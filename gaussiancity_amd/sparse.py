"""Sparse operators of the PTv3 point backbone over libgcs_hip.so.

  SparseConvTensor, SparseModule, SubMConv3d   spconv 2.x (`import spconv.pytorch as spconv`) as models/pt_v3.py
                                               uses them: submanifold convolution only
  segment_csr                                  torch_scatter.segment_csr with a 1-D indptr (reduction along dim 0)

torch supplies device memory (the caching allocator), autograd plumbing and the current stream; the computation
is in the HIP library.  float32 (the default of everything) and float16.  Semantics that spconv leaves open are fixed here:
  * several rows on one voxel: the lowest row is the voxel's representative, every row of the voxel gets the same
    output, and only representatives are read as neighbours;
  * min / max of segment_csr: the gradient goes to the first row that attains the value.

Two engines run the three products of the convolution, the forward, dX and dW (include/gcs.h, ABI v4): "valu", the
default, and "mfma", the same products on the f32 matrix cores, the forward and dX cut over the taps where the grid is
small.  set_engine() / get_engine() choose for the convolutions that start afterwards; the environment variable
GCS_ENGINE gives the initial value; engine_products() says which products an engine runs on the matrix cores.

float16 (dtypes(); the `_t` entry points of include/gcs.h): a layer whose features, weight and bias are float16
(`module.half()`) runs its three products on the f16 matrix cores with fp32 accumulation and one rounding on store; there is
one engine for it, so set_engine() and GCS_ENGINE do not affect such a layer.  Under CUDA autocast, whatever its dtype,
SubMConv3d casts features, weight and bias to float16 for the call and returns float16, as spconv does
(custom_fwd(cast_inputs=torch.float16)).  segment_csr dispatches on src.dtype and has no autocast rule, as upstream.
"""
import ctypes as C
import functools
import math
import os

import torch

from . import _native_s as S
from ._loader import current_stream as _stream

_STATS = {"rulebook_builds": 0, "conv_forward_calls_valu": 0, "conv_forward_calls_mfma": 0, "conv_dw_calls_valu": 0,
          "conv_dw_calls_mfma": 0, "conv_forward_calls_half": 0, "conv_dw_calls_half": 0}
_DTYPES = {torch.float32: "float32", torch.float16: "float16"}


def stats():
    """Counters of this process: `rulebook_builds` counts rulebooks built (a reused indice_key does not build),
    `conv_forward_calls_valu` / `conv_forward_calls_mfma` the convolution forwards each engine ran,
    `conv_dw_calls_valu` / `conv_dw_calls_mfma` the weight gradients each engine ran (a backward that is not asked
    for the weight gradient counts nothing).  `conv_forward_calls_half` / `conv_dw_calls_half` count the float16 calls,
    which the four engine counters do not."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _engine_name(name, where):
    if name not in S.ENGINES:
        raise ValueError("%s: the engine must be \"valu\" or \"mfma\", got %r" % (where, name))
    return name


_ENGINE = _engine_name(os.environ.get("GCS_ENGINE", "valu"), "GCS_ENGINE")


def get_engine():
    """The engine that the next SubMConv3d forward will run (and with it that layer's backward): "valu" or "mfma"."""
    return _ENGINE


def set_engine(name):
    """Choose "valu" or "mfma" for the convolutions whose forward starts from now on; returns the previous name."""
    global _ENGINE
    prev, _ENGINE = _ENGINE, _engine_name(name, "set_engine")
    return prev


_PRODUCTS = (("forward", S.PRODUCT_FORWARD), ("dx", S.PRODUCT_DX), ("dw", S.PRODUCT_DW))


def engine_products(name=None):
    """The products that engine `name` (the current engine when None) runs on the matrix cores, a tuple of names out of
    ("forward", "dx", "dw"): () for "valu", all three for "mfma" (gcs_engine_products)."""
    bits = S.engine_products(S.ENGINES[_engine_name(_ENGINE if name is None else name, "engine_products")])
    return tuple(product for product, bit in _PRODUCTS if bits & bit)


def dtypes():
    """The feature dtypes the library runs (gcs_dtypes): ("float32", "float16")."""
    return S.dtypes()


@functools.lru_cache(maxsize=256)
def _half_workspace_bytes(n, cin, cout, kvol, dups):
    return S.subm_workspace_bytes_t(S.DTYPE_F16, n, cin, cout, kvol, dups)


@functools.lru_cache(maxsize=256)
def _mfma_workspace_bytes(n, cin, cout, kvol, dups):
    return S.subm_engine_workspace_bytes(S.ENGINE_MFMA, n, cin, cout, kvol, dups)


def _valu_workspace_bytes(n, cin, cout, kvol, dups):
    return 0, S.lib().gcs_subm_backward_workspace_bytes(n, cin, cout, kvol, dups)


# The routes of SubMConvFunction, by the suffix of their `_STATS` keys: the suffix of gcs_subm_forward / gcs_subm_backward,
# the leading engine / dtype argument of those entry points, the workspace query -> (forward bytes, backward bytes).
_ROUTES = {"valu": ("", (), _valu_workspace_bytes),
           "mfma": ("_engine", (S.ENGINE_MFMA,), _mfma_workspace_bytes),
           "half": ("_t", (S.DTYPE_F16,), _half_workspace_bytes)}


def _triple(v, name):
    t = tuple(int(a) for a in v) if isinstance(v, (tuple, list)) else (int(v),) * 3
    if len(t) != 3:
        raise ValueError("%s must be an int or three ints, got %r" % (name, v))
    return t


class Rulebook:
    """Neighbour map of one set of indices for one kernel size and dilation (include/gcs.h).  `pairs[k]` is the
    number of rows that have tap k; `dups` says whether some voxel holds several rows."""
    __slots__ = ("buf", "n", "ksize", "dilation", "kvol", "dups", "pairs", "indices")

    def __init__(self, indices, spatial_shape, batch_size, ksize, dilation):
        L = S.lib()
        n = int(indices.shape[0])
        kvol = ksize[0] * ksize[1] * ksize[2]
        shape = _triple(spatial_shape, "spatial_shape")
        if min(shape) < 1 or int(batch_size) < 1:
            raise ValueError("spatial_shape %r and batch_size %r must be positive" % (shape, batch_size))
        if max(shape) >= 2 ** 31 or int(batch_size) * shape[0] * shape[1] * shape[2] > 2 ** 63:
            raise ValueError("batch_size * spatial_shape (%d * %r) does not fit the 64-bit voxel key" % (batch_size, shape))
        rb_bytes = L.gcs_subm_rulebook_bytes(n, kvol)
        sc_bytes = L.gcs_subm_rulebook_scratch_bytes(n)
        if rb_bytes == 0 or sc_bytes == 0:
            raise ValueError(L.gcs_last_error().decode())
        dev = indices.device
        self.buf = torch.empty(rb_bytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(sc_bytes, dtype=torch.uint8, device=dev)
        info = (C.c_int32 * (S.HOST_INFO_HEADER + kvol))()
        with torch.cuda.device(dev):
            S.check(L.gcs_subm_rulebook(indices.data_ptr() if n else None, n, int(batch_size), S.triple(shape),
                                        S.triple(ksize), S.triple(dilation), self.buf.data_ptr(), rb_bytes,
                                        scratch.data_ptr(), sc_bytes, info, _stream()), "gcs_subm_rulebook")
        _STATS["rulebook_builds"] += 1
        if info[0]:
            raise ValueError("%d of %d indices rows are outside batch_size %d x spatial_shape %r"
                             % (info[0], n, batch_size, list(shape)))
        self.n, self.ksize, self.dilation, self.kvol = n, ksize, dilation, kvol
        self.dups = int(info[1])
        self.pairs = [int(info[S.HOST_INFO_HEADER + k]) for k in range(kvol)]
        self.indices = indices


class SparseConvTensor:
    """spconv.SparseConvTensor: features [N, C] float32 or float16, indices [N, 4] int32 (b, d0, d1, d2)."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None, voxel_num=None, indice_dict=None,
                 benchmark=False, permanent_thrust_allocator=False, enable_timer=False, force_algo=None):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {} if indice_dict is None else indice_dict
        self.grid = grid
        self.voxel_num = voxel_num
        self.benchmark = benchmark

    def replace_feature(self, feature):
        """A tensor with new features that shares indices and the indice_dict object (and so its rulebooks)."""
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.grid, self.voxel_num,
                                self.indice_dict, self.benchmark)

    @property
    def spatial_size(self):
        return self.spatial_shape[0] * self.spatial_shape[1] * self.spatial_shape[2]

    def find_indice_pair(self, key):
        return self.indice_dict.get(key) if key is not None else None

    def dense(self, channels_first=True):
        """[B, C, D0, D1, D2] (channels_first) or [B, D0, D1, D2, C]; rows on one voxel: the last write wins."""
        C_ = self.features.shape[1]
        out = self.features.new_zeros([self.batch_size] + self.spatial_shape + [C_])
        idx = self.indices.long()
        out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = self.features
        return out.permute(0, 4, 1, 2, 3).contiguous() if channels_first else out


class SparseModule(torch.nn.Module):
    """Base class of the modules that take and return a SparseConvTensor (spconv.SparseModule)."""


def is_spconv_module(module):
    return isinstance(module, SparseModule)


class SubMConvFunction(torch.autograd.Function):
    """(features [N, Cin], weight [Cout, kD, kH, kW, Cin], bias [Cout] or None, Rulebook) -> [N, Cout]."""

    @staticmethod
    def forward(ctx, features, weight, bias, rb):
        x = features.contiguous()
        w = weight.contiguous()
        n, cin, cout = x.shape[0], x.shape[1], w.shape[0]
        out = x.new_empty((n, cout))
        # read once: the backward of this call runs the same engine, whatever is set by then; float16 has one engine
        engine = "half" if x.dtype == torch.float16 else _ENGINE
        suffix, lead, workspace_bytes = _ROUTES[engine]
        name = "gcs_subm_forward" + suffix
        ws_args = ()  # the plain forward takes no workspace
        if lead:
            ws_bytes = workspace_bytes(n, cin, cout, rb.kvol, rb.dups)[0]
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
            ws_args = (ws.data_ptr() if ws is not None else None, ws_bytes)
        b_ptr = bias.contiguous().data_ptr() if bias is not None else None
        with torch.cuda.device(x.device):
            S.check(getattr(S.lib(), name)(*lead, rb.buf.data_ptr(), n, rb.kvol, x.data_ptr() if n else None, cin,
                                           w.data_ptr(), b_ptr, cout, out.data_ptr() if n else None, *ws_args, _stream()),
                    name)
        _STATS["conv_forward_calls_" + engine] += 1
        ctx.save_for_backward(x, w)
        ctx.rb = rb
        ctx.engine = engine
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w = ctx.saved_tensors
        rb = ctx.rb
        dy = dout.contiguous().to(x.dtype)
        n, cin, cout = x.shape[0], x.shape[1], w.shape[0]
        want_x, want_w, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = x.new_empty(x.shape) if want_x else None
        dw = w.new_empty(w.shape) if want_w else None
        db = w.new_empty((cout,)) if want_b else None
        ptr = lambda t: t.data_ptr() if (t is not None and t.numel()) else None  # noqa: E731
        suffix, lead, workspace_bytes = _ROUTES[ctx.engine]
        name = "gcs_subm_backward" + suffix
        ws_bytes = workspace_bytes(n, cin, cout, rb.kvol, rb.dups)[1]
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            S.check(getattr(S.lib(), name)(*lead, rb.buf.data_ptr(), n, rb.kvol, rb.dups, ptr(x), cin, w.data_ptr(), cout,
                                           ptr(dy), ptr(dx), ptr(dw), ptr(db), ws.data_ptr(), ws_bytes, _stream()), name)
        if want_w:
            _STATS["conv_dw_calls_" + ctx.engine] += 1
        return dx, dw, db, None


class SubMConv3d(SparseModule):
    """spconv.SubMConv3d: submanifold 3-D convolution; output rows are the input rows.

    weight [out, kD, kH, kW, in] (spconv 2.x KRSC), bias [out] or None.  Odd kernel sizes only; stride and groups
    must be 1; padding, algo and fp32_accum are accepted and ignored (the centre tap is kernel_size // 2).

    float32 or float16: features, weight and bias share one dtype (`module.half()` for float16).  While CUDA autocast is
    enabled, whatever its dtype, the three are cast to float16 for the call, from any floating dtype (the bfloat16 a
    Linear emits under bfloat16 autocast included), and the output is float16, as spconv does; float32 parameters then
    receive float32 gradients through the cast.  Outside autocast bfloat16 and float64 are a TypeError."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, algo=None, fp32_accum=None, large_kernel_fast_algo=False, name=None):
        super().__init__()
        ks = _triple(kernel_size, "kernel_size")
        if any(k < 1 or k % 2 == 0 for k in ks):
            raise ValueError("SubMConv3d needs odd kernel sizes, got %r" % (kernel_size,))
        if any(s != 1 for s in _triple(stride, "stride")):
            raise ValueError("SubMConv3d supports stride 1 only, got %r" % (stride,))
        if groups != 1:
            raise ValueError("SubMConv3d supports groups=1 only, got %r" % (groups,))
        dl = _triple(dilation, "dilation")
        if any(d < 1 for d in dl):
            raise ValueError("dilation must be positive, got %r" % (dilation,))
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.dilation, self.stride = ks, dl, (1, 1, 1)
        self.padding = padding
        self.groups = 1
        self.subm = True
        self.indice_key = indice_key
        self.algo, self.fp32_accum, self.name = algo, fp32_accum, name
        self.weight = torch.nn.Parameter(torch.empty(self.out_channels, *ks, self.in_channels))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        fan_in = self.in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
        bound = 1.0 / fan_in ** 0.5
        torch.nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            torch.nn.init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return "%d, %d, kernel_size=%r, dilation=%r, bias=%s, indice_key=%r" % (
            self.in_channels, self.out_channels, self.kernel_size, self.dilation, self.bias is not None, self.indice_key)

    def _rulebook(self, x):
        key = self.indice_key
        rb = x.indice_dict.get(key) if key is not None else None
        if rb is not None:
            if not isinstance(rb, Rulebook) or rb.ksize != self.kernel_size or rb.dilation != self.dilation:
                raise ValueError("indice_key %r was built for kernel_size %r, dilation %r; this layer has %r, %r"
                                 % (key, getattr(rb, "ksize", None), getattr(rb, "dilation", None), self.kernel_size,
                                    self.dilation))
            if rb.n != x.indices.shape[0]:
                raise ValueError("indice_key %r was built for %d rows, the tensor has %d" % (key, rb.n, x.indices.shape[0]))
            return rb
        rb = Rulebook(x.indices, x.spatial_shape, x.batch_size, self.kernel_size, self.dilation)
        if key is not None:
            x.indice_dict[key] = rb
        return rb

    def forward(self, x):
        f, idx = x.features, x.indices
        w, b = self.weight, self.bias
        given = [t.dtype for t in (f, w, b) if t is not None]
        autocast = torch.is_autocast_enabled()
        # under autocast every floating dtype is cast to float16 below (custom_fwd casts bfloat16 and float64 too)
        if any(not d.is_floating_point if autocast else d not in _DTYPES for d in given):
            raise TypeError("SubMConv3d supports float32 and float16 only (features %s, weight %s)" % (f.dtype, w.dtype))
        if not autocast and len(set(given)) != 1:
            raise TypeError("SubMConv3d needs features, weight and bias of one dtype, float32 or float16, outside autocast "
                            "(features %s, weight %s%s)" % (f.dtype, w.dtype, "" if b is None else ", bias %s" % b.dtype))
        if idx.dtype != torch.int32:
            raise TypeError("indices must be int32, got %s" % idx.dtype)
        if f.dim() != 2 or idx.dim() != 2 or idx.shape[1] != 4 or f.shape[0] != idx.shape[0]:
            raise ValueError("features [N, C] and indices [N, 4] expected, got %r and %r" % (tuple(f.shape), tuple(idx.shape)))
        if f.shape[1] != self.in_channels:
            raise ValueError("features have %d channels, the layer expects %d" % (f.shape[1], self.in_channels))
        if not f.is_cuda or not idx.is_cuda:
            raise RuntimeError("SubMConv3d runs on the GPU; features and indices must be CUDA tensors")
        if not idx.is_contiguous():
            x = SparseConvTensor(f, idx.contiguous(), x.spatial_shape, x.batch_size, indice_dict=x.indice_dict)
        rb = self._rulebook(x)
        if not autocast:
            return x.replace_feature(SubMConvFunction.apply(f, w, b, rb))
        # spconv's custom_fwd(cast_inputs=torch.float16): float16 operands, the call itself outside autocast
        half = lambda t: None if t is None else t.to(torch.float16)  # noqa: E731
        with torch.autocast("cuda", enabled=False):
            return x.replace_feature(SubMConvFunction.apply(half(f), half(w), half(b), rb))


class SegmentCSRFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, indptr, reduce):
        x = src.contiguous()
        ip = indptr.contiguous()
        m, nseg = x.shape[0], ip.shape[0] - 1
        f = math.prod(x.shape[1:])
        out = x.new_empty((nseg,) + tuple(x.shape[1:]))
        code = S.REDUCE[reduce]
        dtype = S.DTYPES[_DTYPES[x.dtype]]
        arg = torch.empty((nseg, f), dtype=torch.int64, device=x.device) if code >= 2 else None
        if nseg and f:
            with torch.cuda.device(x.device):
                S.check(S.lib().gcs_segment_csr_forward_t(dtype, x.data_ptr() if m else None, m, f, ip.data_ptr(), nseg, code,
                                                          out.data_ptr(), arg.data_ptr() if arg is not None else None,
                                                          _stream()), "gcs_segment_csr_forward_t")
        ctx.save_for_backward(ip, arg) if arg is not None else ctx.save_for_backward(ip)
        ctx.meta = (tuple(x.shape), m, f, nseg, code, x.dtype)
        if arg is not None:
            ctx.mark_non_differentiable(arg)
        return out

    @staticmethod
    def backward(ctx, dout):
        shape, m, f, nseg, code, dt = ctx.meta
        saved = ctx.saved_tensors
        ip, arg = saved[0], (saved[1] if len(saved) > 1 else None)
        dy = dout.contiguous().to(dt)
        dsrc = dy.new_zeros(shape) if not (m and f) else dy.new_empty(shape)
        if m and f:
            with torch.cuda.device(dy.device):
                S.check(S.lib().gcs_segment_csr_backward_t(S.DTYPES[_DTYPES[dt]], dy.data_ptr() if nseg else None, m, f,
                                                           ip.data_ptr(), nseg, code,
                                                           arg.data_ptr() if arg is not None else None, dsrc.data_ptr(),
                                                           _stream()), "gcs_segment_csr_backward_t")
        return dsrc, None, None


def segment_csr(src, indptr, out=None, reduce="sum"):
    """torch_scatter.segment_csr for a 1-D int64 indptr: reduces float32 or float16 `src` along dim 0 over the rows
    [indptr[s], indptr[s+1]) of every segment s.  reduce: sum / add / mean / min / max; an empty segment gives 0."""
    if out is not None:
        raise NotImplementedError("segment_csr(out=...) is not supported")
    if indptr.dim() != 1:
        raise NotImplementedError("segment_csr supports a 1-D indptr only (got %d-D)" % indptr.dim())
    if reduce not in S.REDUCE:
        raise ValueError("reduce must be one of sum, add, mean, min, max (got %r)" % (reduce,))
    if src.dtype not in _DTYPES:
        raise TypeError("segment_csr supports float32 and float16 src only (got %s)" % src.dtype)
    if indptr.dtype != torch.int64:
        raise TypeError("indptr must be int64 (got %s)" % indptr.dtype)
    if src.dim() < 1 or indptr.numel() < 1:
        raise ValueError("src needs at least one dimension and indptr at least one entry")
    if not src.is_cuda or not indptr.is_cuda:
        raise RuntimeError("segment_csr runs on the GPU; src and indptr must be CUDA tensors")
    return SegmentCSRFunction.apply(src, indptr, reduce)
