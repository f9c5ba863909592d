"""SerializedPooling and SerializedUnpooling of the PTv3 point backbone over libgcs_hip.so (include/gcs.h, DESIGN.md
section 15.6): the cluster plan of a pooling stage as kernels, and a row-indexed segment reduce, so that neither
`feat[indices]` nor `feat[inverse]` is materialised and no backward sorts indices for an index_put.

  pool_plan(code, pooling_depth)       PoolPlan of the point set's serialized_code [k, n]: one host wait, for S
  pooled_reduce(src, plan, reduce)     segment_csr(src[plan.indices], plan.idx_ptr, reduce) bit for bit, src read in place
  gather_forward / gather_backward     the two calls under it, without autograd
  unpool_add(parent, child, plan)      parent + child[plan.cluster] in one pass; d_child is a pooled_reduce sum of dout
  install(pt_v3) / uninstall(pt_v3)    rebind SerializedPooling.forward and SerializedUnpooling.forward of a caller's
                                       imported models.pt_v3

torch supplies device memory and the current stream; the computation is in the HIP library, and there is no other path
for CUDA tensors: a failing call raises.  The plan's integers are exact.  `indices` lists the rows by cluster with ties to
the lower row (torch.sort(stable=True)); upstream's torch.sort leaves ties open, and `head` and the fp32 sum order hang on
them.  Neither autograd.Function waits for the device, forward or backward, and every gradient is bit-identical from run
to run: no float atomics, every element written exactly once.
"""
import math
import threading

import torch

from . import _native_s as S
from . import point_seam
from ._loader import current_stream as _stream

REDUCES = ("sum", "mean", "min", "max")
_DTYPES = {torch.float32: S.DTYPE_F32, torch.float16: S.DTYPE_F16}
_STATS = {"plan_calls": 0, "reduce_calls": 0, "reduce_backward_calls": 0, "unpool_calls": 0, "pooling_fused": 0,
          "pooling_original": 0, "unpooling_fused": 0, "unpooling_original": 0}
_ORIGINALS = "_gaussiancity_amd_point_pool_originals"
_local = threading.local()

FIELDS = ("cluster", "indices", "idx_ptr", "head", "code", "order", "inverse", "n", "s")


class PoolPlan:
    """cluster [n], indices [n], idx_ptr [s + 1], head [s], code / order / inverse [k, s] (the pooled point set's
    serialized keys), all int64 on the code's device; n and s are Python ints.  (An object and no tuple: addict.Dict,
    which upstream's Point is, rebuilds every tuple it is handed.)"""
    __slots__ = FIELDS

    def __init__(self, cluster, indices, idx_ptr, head, code, order, inverse, n, s):
        self.cluster, self.indices, self.idx_ptr, self.head = cluster, indices, idx_ptr, head
        self.code, self.order, self.inverse, self.n, self.s = code, order, inverse, int(n), int(s)


def stats():
    """Counters of this process: the calls that reached the library, and the path each rebound forward took."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def reduces():
    """The reduce names the gathered reduce runs (gcs_pool_reduces), in enum order."""
    bits = S.lib().gcs_pool_reduces()
    return tuple(name for name in REDUCES if bits >> S.REDUCE[name] & 1)


def _cuda(t, name, where):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError("%s: %s must be a CUDA tensor (there is no CPU path)" % (where, name))


def _pinned_count():
    """One pinned int64 word of this thread: gcs_pool_plan_count's S."""
    buf = getattr(_local, "count", None)
    if buf is None:
        buf = _local.count = torch.empty(1, dtype=torch.int64).pin_memory()
    return buf


def pool_plan(code, pooling_depth):
    """PoolPlan for `code` int64 [k, n] (a point set's serialized_code, k in 1...5) and the stage's pooling depth
    (0...16): clusters are the distinct values of code[0] >> 3 * pooling_depth in ascending order.  One host wait."""
    _cuda(code, "code", "pool_plan")
    if code.dim() != 2 or code.dtype != torch.int64 or code.shape[1] < 1:
        raise ValueError("pool_plan: code must be a non-empty int64 tensor [k, n], got %s %s" % (code.dtype, tuple(code.shape)))
    dev, k, n = code.device, int(code.shape[0]), int(code.shape[1])
    shift = 3 * int(pooling_depth)
    c = code.contiguous()
    L, count = S.lib(), _pinned_count()
    ws_bytes = L.gcs_pool_plan_workspace_bytes(n, k)
    if not ws_bytes:
        raise ValueError("pool_plan: %s" % L.gcs_last_error().decode())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        S.check(L.gcs_pool_plan_count(c.data_ptr(), k, n, shift, ws.data_ptr(), ws_bytes, count.data_ptr(), _stream()),
                "gcs_pool_plan_count")
        s = int(count[0])
        rows = torch.empty(2 * n, dtype=torch.int64, device=dev)  # cluster, indices
        segs = torch.empty(2 * s + 1, dtype=torch.int64, device=dev)  # idx_ptr, head
        down = torch.empty((3, k, s), dtype=torch.int64, device=dev)  # code, order, inverse
        cluster, indices, idx_ptr, head = rows[:n], rows[n:], segs[:s + 1], segs[s + 1:]
        S.check(L.gcs_pool_plan_emit(c.data_ptr(), k, n, shift, s, ws.data_ptr(), ws_bytes, cluster.data_ptr(),
                                     indices.data_ptr(), idx_ptr.data_ptr(), head.data_ptr(), down[0].data_ptr(),
                                     down[1].data_ptr(), down[2].data_ptr(), _stream()), "gcs_pool_plan_emit")
    _STATS["plan_calls"] += 1
    return PoolPlan(cluster, indices, idx_ptr, head, down[0], down[1], down[2], n, s)


def _rows(t):
    """`t` [n, ...] as (tensor, row stride in elements, f): in place when only the rows are strided, else a copy."""
    f = math.prod(t.shape[1:])
    flat = t if t.dim() == 2 else t.reshape(t.shape[0], f)
    if f == 0 or flat.shape[0] == 0:
        return flat.contiguous(), f, f
    if flat.stride(1) != 1 and f > 1 or flat.stride(0) < f:
        flat = flat.contiguous()
    return flat, int(flat.stride(0)), f


def gather_forward(src, plan, reduce):
    """(out [s, f], arg int64 [s, f] or None) of gcs_segment_gather_forward_t for src [n, f]: the call under
    pooled_reduce, without autograd.  arg (min and max) holds SOURCE rows, -1 for an empty segment."""
    x, stride, f = _rows(src)
    code = S.REDUCE[reduce]
    out = torch.empty((plan.s, f), dtype=x.dtype, device=x.device)
    arg = torch.empty((plan.s, f), dtype=torch.int64, device=x.device) if code >= 2 else None
    with torch.cuda.device(x.device):
        S.check(S.lib().gcs_segment_gather_forward_t(_DTYPES[x.dtype], x.data_ptr(), stride, plan.n, f,
                                                     plan.indices.data_ptr(), plan.idx_ptr.data_ptr(), plan.s, code,
                                                     out.data_ptr(), arg.data_ptr() if arg is not None else None, _stream()),
                "gcs_segment_gather_forward_t")
    return out, arg


def gather_backward(dout, plan, reduce, arg=None, out=None):
    """dsrc [n, f] of gcs_segment_gather_backward_t for dout [s, f] (contiguous): the call under pooled_reduce's
    backward.  `out`, when given, is a [n, f] tensor with unit column stride that the call overwrites entirely."""
    f = int(dout.shape[1])
    dsrc = torch.empty((plan.n, f), dtype=dout.dtype, device=dout.device) if out is None else out
    with torch.cuda.device(dout.device):
        S.check(S.lib().gcs_segment_gather_backward_t(_DTYPES[dout.dtype], dout.data_ptr(), plan.n, f,
                                                      plan.cluster.data_ptr(), plan.idx_ptr.data_ptr(), plan.s,
                                                      S.REDUCE[reduce], arg.data_ptr() if arg is not None else None,
                                                      dsrc.data_ptr(), int(dsrc.stride(0)), _stream()),
                "gcs_segment_gather_backward_t")
    return dsrc


class PooledReduceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, plan, reduce):
        out, arg = gather_forward(src.detach(), plan, reduce)
        _STATS["reduce_calls"] += 1
        ctx.plan, ctx.meta, ctx.arg = plan, (tuple(src.shape), reduce, src.dtype), arg
        return out.view((plan.s,) + tuple(src.shape[1:]))

    @staticmethod
    def backward(ctx, dout):
        plan, (shape, reduce, dt), arg = ctx.plan, ctx.meta, ctx.arg
        dy = dout.to(dt).reshape(plan.s, -1).contiguous()
        dsrc = gather_backward(dy, plan, reduce, arg)
        _STATS["reduce_backward_calls"] += 1
        return dsrc.view(shape), None, None


def _check_plan(plan, where):
    if not isinstance(plan, PoolPlan):
        raise TypeError("%s: plan must be a PoolPlan (pool_plan's result)" % where)


def pooled_reduce(src, plan, reduce="sum"):
    """segment_csr(src[plan.indices], plan.idx_ptr, reduce) without the gathered copy: src [n, ...] float32 or float16,
    its rows may be strided (a column slice of a wider tensor is read in place); the result is [s, ...].  Sum and mean
    are one fp32 chain per element in ascending position of plan.indices, rounded once; min and max send the gradient to
    the first row that attains the value.  No host wait, forward or backward."""
    _cuda(src, "src", "pooled_reduce")
    _check_plan(plan, "pooled_reduce")
    if reduce not in REDUCES:
        raise ValueError("pooled_reduce: reduce must be one of %s (got %r)" % (", ".join(REDUCES), reduce))
    if src.dtype not in _DTYPES:
        raise TypeError("pooled_reduce: src must be float32 or float16 (got %s)" % src.dtype)
    if src.dim() < 2 or src.shape[0] != plan.n or math.prod(src.shape[1:]) < 1:
        raise ValueError("pooled_reduce: src must be [n = %d, ...] with at least one column, got %s" % (plan.n, tuple(src.shape)))
    return PooledReduceFunction.apply(src, plan, reduce)


class UnpoolAddFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, parent, child, plan):
        b = child.detach().contiguous()
        a = parent.detach().contiguous() if parent is not None else None
        f = int(b.shape[1])
        out = torch.empty((plan.n, f), dtype=b.dtype, device=b.device)
        with torch.cuda.device(b.device):
            S.check(S.lib().gcs_segment_expand_add_t(_DTYPES[b.dtype], a.data_ptr() if a is not None else None, b.data_ptr(),
                                                     plan.cluster.data_ptr(), plan.n, f, out.data_ptr(), _stream()),
                    "gcs_segment_expand_add_t")
        _STATS["unpool_calls"] += 1
        ctx.plan, ctx.has_parent = plan, parent is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        plan = ctx.plan
        d_child = gather_forward(dout, plan, "sum")[0] if ctx.needs_input_grad[1] else None
        return (dout if ctx.has_parent and ctx.needs_input_grad[0] else None), d_child, None


def unpool_add(parent_feat, child_feat, plan):
    """parent_feat [n, f] + child_feat [s, f][plan.cluster] in one pass (one fp32 add, rounded once); parent_feat None
    gives the plain expansion.  Backward: d_parent is dout, d_child the pooled_reduce sum of dout -- each row of d_child
    one fp32 chain over its cluster's rows in ascending row order."""
    _cuda(child_feat, "child_feat", "unpool_add")
    _check_plan(plan, "unpool_add")
    if child_feat.dtype not in _DTYPES:
        raise TypeError("unpool_add: child_feat must be float32 or float16 (got %s)" % child_feat.dtype)
    if child_feat.dim() != 2 or child_feat.shape[0] != plan.s or child_feat.shape[1] < 1:
        raise ValueError("unpool_add: child_feat must be [s = %d, f], got %s" % (plan.s, tuple(child_feat.shape)))
    if parent_feat is not None:
        _cuda(parent_feat, "parent_feat", "unpool_add")
        if parent_feat.dtype != child_feat.dtype or parent_feat.device != child_feat.device:
            raise TypeError("unpool_add: parent_feat and child_feat must share dtype and device")
        if tuple(parent_feat.shape) != (plan.n, child_feat.shape[1]):
            raise ValueError("unpool_add: parent_feat must be [n = %d, %d], got %s"
                             % (plan.n, child_feat.shape[1], tuple(parent_feat.shape)))
    return UnpoolAddFunction.apply(parent_feat, child_feat, plan)


# ---- the two forwards of models/pt_v3.py, written against their behaviour: the keys they read and write, their
# assertions, the host generator's one draw under shuffle_orders, and the norm / act / sparsify tail ------------------
def _fused(*tensors):
    return all(t.is_cuda for t in tensors) and all(t.dtype in _DTYPES for t in tensors if t.is_floating_point())


def _pooling_forward(original, point_class, pt_v3_module):
    def forward(self, point):
        """SerializedPooling.forward over gcs_pool_plan_* and the gathered reduce; a point set on the CPU or in another
        dtype than float32 / float16 goes to the original method.  With point_seam's marker on the module, the norm / act
        tail is one fused call when the two containers are that pair."""
        pooling_depth = (math.ceil(self.stride) - 1).bit_length()
        if pooling_depth > point.serialized_depth:
            pooling_depth = 0
        assert {"serialized_code", "serialized_order", "serialized_inverse", "serialized_depth"}.issubset(
            point.keys()), "Run point.serialization() point cloud before SerializedPooling"
        if not _fused(point.serialized_code, point.feat, point.coord, self.proj.weight):
            _STATS["pooling_original"] += 1
            return original(self, point)
        feat = self.proj(point.feat)
        if feat.dtype not in _DTYPES:  # an autocast dtype the library does not run
            _STATS["pooling_original"] += 1
            return original(self, point)
        plan = pool_plan(point.serialized_code, pooling_depth)
        code, order, inverse = plan.code, plan.order, plan.inverse
        if self.shuffle_orders:
            perm = torch.randperm(code.shape[0])
            code, order, inverse = code[perm], order[perm], inverse[perm]
        point_dict = dict(
            feat=pooled_reduce(feat, plan, self.reduce),
            coord=pooled_reduce(point.coord, plan, "mean"),
            grid_coord=point.grid_coord[plan.head] >> pooling_depth,
            serialized_code=code,
            serialized_order=order,
            serialized_inverse=inverse,
            serialized_depth=point.serialized_depth - pooling_depth,
            batch=point.batch[plan.head],
        )
        if "condition" in point.keys():
            point_dict["condition"] = point.condition
        if "context" in point.keys():
            point_dict["context"] = point.context
        if self.traceable:
            point_dict["pooling_inverse"] = plan.cluster
            point_dict["pooling_parent"] = point
            point_dict["pooling_plan"] = plan
        _STATS["pooling_fused"] += 1
        point = point_class(point_dict)
        if (getattr(pt_v3_module, point_seam._MARK, False) and self.norm is not None and self.act is not None
                and point.feat.size(0) != 1 and point_seam.pooling_tail(self.norm, self.act, point)):
            point.sparsify()
            return point
        if self.norm is not None and point.feat.size(0) != 1:
            point = self.norm(point)
        if self.act is not None:
            point = self.act(point)
        point.sparsify()
        return point
    return forward


def _unpooling_forward(original):
    def forward(self, point):
        """SerializedUnpooling.forward over gcs_segment_expand_add_t; without the pooling's plan on the point, on the
        CPU, or with features of two dtypes, the original method runs."""
        assert "pooling_parent" in point.keys()
        assert "pooling_inverse" in point.keys()
        plan = point.pop("pooling_plan", None) if "pooling_plan" in point.keys() else None
        if plan is None:
            _STATS["unpooling_original"] += 1
            return original(self, point)
        parent = point.pop("pooling_parent")
        inverse = point.pop("pooling_inverse")
        point = self.proj(point)
        parent = self.proj_skip(parent)
        a, b = parent.feat, point.feat
        if _fused(a, b) and a.dtype == b.dtype and a.dim() == 2 and b.dim() == 2:
            parent.feat = unpool_add(a, b, plan)
            _STATS["unpooling_fused"] += 1
        else:
            parent.feat = a + b[inverse]
            _STATS["unpooling_original"] += 1
        if self.traceable:
            parent["unpooling_parent"] = point
        return parent
    return forward


def install(pt_v3_module):
    """Rebind SerializedPooling.forward and SerializedUnpooling.forward of the caller's imported models.pt_v3 to the
    library.  Idempotent, and independent of point_index.install and point_attention.install; uninstall() puts the
    module's own methods back."""
    if getattr(pt_v3_module, _ORIGINALS, None) is not None:
        return
    reduces()  # loads the library: a build without the pooling entry points fails here, not inside a forward
    pooling, unpooling = pt_v3_module.SerializedPooling, pt_v3_module.SerializedUnpooling
    originals = (pooling.forward, unpooling.forward)
    setattr(pt_v3_module, _ORIGINALS, originals)
    pooling.forward = _pooling_forward(originals[0], pt_v3_module.Point, pt_v3_module)
    unpooling.forward = _unpooling_forward(originals[1])


def uninstall(pt_v3_module):
    originals = getattr(pt_v3_module, _ORIGINALS, None)
    if originals is None:
        return
    pt_v3_module.SerializedPooling.forward, pt_v3_module.SerializedUnpooling.forward = originals
    delattr(pt_v3_module, _ORIGINALS)
