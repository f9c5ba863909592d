"""Index plans of the PTv3 point backbone over libgcs_hip.so (include/gcs.h): what
models/pt_v3.py builds between its kernels with host-driven torch glue, as kernels.

  serialize(grid_coord, batch, depth, orders)   Point.serialization's codes, order and inverse, for every requested
                                                order in one call: no host wait
  patch_plan(offset, patch_size)                SerializedAttention.get_padding_and_inverse's pad, unpad and cu_seqlens:
                                                one host wait, for the two output sizes
  install(pt_v3) / uninstall(pt_v3)             rebind those two methods of a caller's imported models.pt_v3

torch supplies device memory and the current stream; the computation is in the HIP library, and there is no other path
for CUDA tensors: a failing call raises.  Results are bit-exact integers.  `order` sorts a code row ascending with ties
to the lower row (torch.sort(stable=True)); upstream's torch.argsort leaves the order of equal codes open.  The `cord`
code divides in binary32 as torch's CPU kernels do (include/gcs.h); a GPU kernel that multiplies by the reciprocal of the
divisor instead gives other codes for some coordinates of 256 and above at grid_size 0.01.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _native_s as S
from ._loader import current_stream as _stream

ORDERS = tuple(S.ORDERS)
_STATS = {"serialize_calls": 0, "patch_plan_calls": 0}
_ORIGINALS = "_gaussiancity_amd_point_index_originals"
_local = threading.local()


def stats():
    """Counters of this process: the calls of serialize() and of patch_plan() that reached the library."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def orders():
    """The order names the library computes (gcs_index_orders), in enum order."""
    bits = S.lib().gcs_index_orders()
    return tuple(name for name, code in S.ORDERS.items() if bits >> code & 1)


def _cuda(t, name, where):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError("%s: %s must be a CUDA tensor (there is no CPU path)" % (where, name))


def serialize(grid_coord, batch, depth, orders, grid_size=0.01, n_batches=1):
    """(code, order, inverse), int64 [len(orders), n] on grid_coord.device.  grid_coord: integer [n, 3] (read as int32);
    batch: integer [n] or None; depth 1...16; orders: distinct names out of ORDERS; grid_size: the `cord` divisor, as
    upstream's Serializator.encode takes it.  n_batches is only checked: 3 * depth + n_batches.bit_length() <= 63."""
    _cuda(grid_coord, "grid_coord", "serialize")
    if grid_coord.dim() != 2 or grid_coord.shape[1] != 3 or grid_coord.is_floating_point():
        raise ValueError("serialize: grid_coord must be an integer tensor [n, 3], got %s %s"
                         % (grid_coord.dtype, tuple(grid_coord.shape)))
    names = [orders] if isinstance(orders, str) else list(orders)
    unknown = [o for o in names if o not in S.ORDERS]
    if unknown:
        raise ValueError("serialize: unknown order %r; the library computes %r" % (unknown[0], ORDERS))
    dev, n, k = grid_coord.device, int(grid_coord.shape[0]), len(names)
    g = grid_coord.to(torch.int32).contiguous()
    b = None
    if batch is not None:
        _cuda(batch, "batch", "serialize")
        if batch.shape != (n,) or batch.device != dev:
            raise ValueError("serialize: batch must be [n] on grid_coord's device")
        b = batch.to(torch.int64).contiguous()
    L = S.lib()
    out = torch.empty((3, k, n), dtype=torch.int64, device=dev)
    ws_bytes = L.gcs_serialize_workspace_bytes(n, k)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    codes = (C.c_int32 * max(k, 1))(*[S.ORDERS[o] for o in names])
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    with torch.cuda.device(dev):
        S.check(L.gcs_serialize(ptr(g), ptr(b) if b is not None else None, n, int(n_batches), int(depth),
                                float(np.float32(float(grid_size) ** 2)), float(np.float32(float(grid_size))), codes, k,
                                ptr(out[0]), ptr(out[1]), ptr(out[2]), ws.data_ptr(), ws_bytes, _stream()), "gcs_serialize")
    _STATS["serialize_calls"] += 1
    return out[0], out[1], out[2]


def _pinned_counts():
    """Three pinned int64 words of this thread: gcs_patch_plan_count's two counts, and offset[-1] next to them."""
    buf = getattr(_local, "counts", None)
    if buf is None:
        buf = _local.counts = torch.empty(3, dtype=torch.int64).pin_memory()
    return buf


def patch_plan(offset, patch_size):
    """(pad int64 [padded], unpad int64 [offset[-1]], cu_seqlens int32) for the inclusive row ends `offset` [batches] of
    a serialized point set and the attention's patch size, as upstream computes them.  One host wait: the copy of
    offset[-1] is queued in front of gcs_patch_plan_count, whose wait then covers all three sizes."""
    _cuda(offset, "offset", "patch_plan")
    if offset.dim() != 1 or offset.numel() < 1 or offset.is_floating_point():
        raise ValueError("patch_plan: offset must be a non-empty 1-D integer tensor")
    dev = offset.device
    off = offset.to(torch.int64).contiguous()
    nb, P = int(off.numel()), int(patch_size)
    L, counts = S.lib(), _pinned_counts()
    with torch.cuda.device(dev):
        counts[2:].copy_(off[-1:], non_blocking=True)
        S.check(L.gcs_patch_plan_count(off.data_ptr(), nb, P, counts.data_ptr(), _stream()), "gcs_patch_plan_count")
        padded, n_cu, total = (int(v) for v in counts.tolist())
        pad = torch.empty(padded, dtype=torch.int64, device=dev)
        unpad = torch.empty(total, dtype=torch.int64, device=dev)
        cu = torch.empty(n_cu, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
        S.check(L.gcs_patch_plan_emit(off.data_ptr(), nb, P, padded, n_cu, ptr(pad), ptr(unpad), ptr(cu), _stream()),
                "gcs_patch_plan_emit")
    _STATS["patch_plan_calls"] += 1
    return pad, unpad, cu


# ---- the two methods of models/pt_v3.py, written against their behaviour: the keys they read and write, their
# assertions, their one wait for the depth, and the host generator's draw for shuffle_orders -------------------------
def _serialization(original):
    def serialization(self, order="z", depth=None, shuffle_orders=False):
        """Point.serialization over gcs_serialize; a point set on the CPU goes to the original method."""
        assert "batch" in self.keys()
        if not self.batch.is_cuda:
            return original(self, order=order, depth=depth, shuffle_orders=shuffle_orders)
        if "grid_coord" not in self.keys():
            assert {"grid_size", "coord"}.issubset(self.keys())
            self["grid_coord"] = torch.div(self.coord - self.coord.min(0)[0], self.grid_size, rounding_mode="trunc").int()
        if depth is None:
            depth = int(self.grid_coord.max()).bit_length()  # the method's one wait
        if depth < 1:  # every coordinate is 0: no curve to follow, and nothing to gain
            return original(self, order=order, depth=depth, shuffle_orders=shuffle_orders)
        self["serialized_depth"] = depth
        assert depth * 3 + len(self.offset).bit_length() <= 63
        assert depth <= 16
        names = list(order)
        for name in names:
            assert name in {"cord", "z", "z-trans", "hilbert", "hilbert-trans"}
        distinct = list(dict.fromkeys(names))
        grid_size = self.grid_size if "cord" in distinct else 0.01
        code, order_, inverse = serialize(self.grid_coord, self.batch, depth, distinct, grid_size, len(self.offset))
        rows = [distinct.index(name) for name in names]
        if shuffle_orders:
            rows = [rows[i] for i in torch.randperm(len(names)).tolist()]
        if rows != list(range(len(distinct))):
            code, order_, inverse = code[rows], order_[rows], inverse[rows]
        self["serialized_code"] = code
        self["serialized_order"] = order_
        self["serialized_inverse"] = inverse
    return serialization


def _get_padding_and_inverse(original):
    @torch.no_grad()
    def get_padding_and_inverse(self, point):
        """SerializedAttention.get_padding_and_inverse over gcs_patch_plan_*; a CPU offset goes to the original."""
        keys = ("pad", "unpad", "cu_seqlens_key")
        if not all(k in point.keys() for k in keys):
            if not point.offset.is_cuda:
                return original(self, point)
            point["pad"], point["unpad"], point["cu_seqlens_key"] = patch_plan(point.offset, self.patch_size)
        return point["pad"], point["unpad"], point["cu_seqlens_key"]
    return get_padding_and_inverse


def install(pt_v3_module):
    """Rebind Point.serialization and SerializedAttention.get_padding_and_inverse of the caller's imported models.pt_v3
    to the library.  Idempotent; uninstall() puts the module's own methods back."""
    if getattr(pt_v3_module, _ORIGINALS, None) is not None:
        return
    orders()  # loads the library: a build without the plans fails here, not inside a forward
    point, attention = pt_v3_module.Point, pt_v3_module.SerializedAttention
    originals = (point.serialization, attention.get_padding_and_inverse)
    setattr(pt_v3_module, _ORIGINALS, originals)
    point.serialization = _serialization(originals[0])
    attention.get_padding_and_inverse = _get_padding_and_inverse(originals[1])


def uninstall(pt_v3_module):
    originals = getattr(pt_v3_module, _ORIGINALS, None)
    if originals is None:
        return
    pt_v3_module.Point.serialization, pt_v3_module.SerializedAttention.get_padding_and_inverse = originals
    delattr(pt_v3_module, _ORIGINALS)
