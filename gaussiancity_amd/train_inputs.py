"""The generator's inputs of a training step on the device, over libgcv_hip.so (include/gcv.h K23, K24; DESIGN.md
section 13e): what core/train.py:207-224 does on the host between the data loader and the generator -- five slices of pts,
instances_to_classes (three or four masks, a deepcopy, masked assignments), get_point_scales, get_one_hot,
get_projection_uv and get_z with torch.unique, one .item() wait, one torch.randn, one host-to-device copy and one N-element
compare per instance -- as one launch, or with style codes one count (the only host wait), one launch and one copy.

  TrainRule / rule_from_cfg(dataset_cfg, scale_factor)   the dataset's constants, as config.py spells them
  RULE_GOOGLE_EARTH(scale_factor=0.65) / RULE_KITTI_360(scale_factor=0.65)   config.py's values
  Workspace(device)                           the presence table between the count and the emit, and the flag word
  prepare(pts, rule, z_dim=None, proj_tlp=None, workspace=None, check=False)   TrainInputs
  get_z(instances, z_dim)                     drop-in for utils.helpers.get_z: a model_inputs.GroupedCodes, the same draws
  install(helpers_module) / uninstall(helpers_module)   rebind get_z alone
  stats() / reset_stats()

The style codes are drawn on the host with upstream's own call in upstream's order -- torch.randn(1, z_dim) per instance,
ascending, from the default CPU generator -- so the generator ends in upstream's state and the codes are upstream's values.
torch supplies device memory and the current stream; every computation is in the HIP library.  There is no CPU path.
"""
import collections
import ctypes as C

import torch

from . import _native_v as V
from ._loader import current_stream as _stream
from ._loader import dense as _dense
from .model_inputs import GroupedCodes

_STATS = {"prepare_calls": 0, "get_z_calls": 0}
_ORIGINAL = "_gaussiancity_amd_train_inputs_original_get_z"


def stats():
    """Counters of this process: calls of prepare and of get_z (the installed one included)."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


# ---- the rule ------------------------------------------------------------------------------------------------------------
TrainRule = collections.namedtuple("TrainRule", "bldg_ins_min bldg_ins_max car_ins_min car_ins_max facade_class roof_class "
                                   "car_class n_classes special_z_classes scale_factor proj_size")
TrainRule.__doc__ = """The constants of core/train.py:207-224: ids in [bldg_ins_min, bldg_ins_max) are facade_class when even and
roof_class when odd; ids in [car_ins_min, car_ins_max) are car_class, applied last (min >= max: no cars); n_classes is the
one-hot's width (1..32); special_z_classes the classes whose z-scale is 1; scale_factor multiplies the point's scale;
proj_size divides the projection coordinates."""


def rule_from_cfg(dataset_cfg, scale_factor):
    """The rule of a dataset node of config.py (cfg.DATASETS.GOOGLE_EARTH, cfg.DATASETS.KITTI_360) and
    cfg.NETWORK.GAUSSIAN.SCALE_FACTOR.  CAR_RANGE and CAR_CLSID are read when the node has them."""
    bldg = dataset_cfg.BLDG_RANGE
    car = getattr(dataset_cfg, "CAR_RANGE", None)
    car_class = getattr(dataset_cfg, "CAR_CLSID", None)
    has_car = car is not None and car_class is not None
    return TrainRule(int(bldg[0]), int(bldg[1]), int(car[0]) if has_car else 0, int(car[1]) if has_car else 0,
                     int(dataset_cfg.BLDG_FACADE_CLSID), int(dataset_cfg.BLDG_ROOF_CLSID), int(car_class) if has_car else 0,
                     int(dataset_cfg.N_CLASSES), tuple(sorted(int(c) for c in dataset_cfg.Z_SCALE_SPECIAL_CLASSES.values())),
                     float(scale_factor), float(dataset_cfg.PROJ_SIZE))


def RULE_GOOGLE_EARTH(scale_factor=0.65):
    """cfg.DATASETS.GOOGLE_EARTH: buildings [100, 32768), facade 2, roof 7, no cars, ROAD 1 / WATER 5 / ZONE 6 flat."""
    return TrainRule(100, 32768, 0, 0, 2, 7, 0, 8, (1, 5, 6), float(scale_factor), 2048.0)


def RULE_KITTI_360(scale_factor=0.65):
    """cfg.DATASETS.KITTI_360: buildings [100, 10000), cars [10000, 16384) -> 3, ROAD 1 / ZONE 6 flat."""
    return TrainRule(100, 10000, 10000, 16384, 2, 7, 3, 8, (1, 6), float(scale_factor), 2048.0)


def _native_rule(rule):
    n = int(rule.n_classes)
    if not 1 <= n <= 32:
        raise ValueError("n_classes must be in [1, 32], got %d" % n)
    special = [int(c) for c in rule.special_z_classes]
    if any(not 0 <= c < 32 for c in special):
        raise ValueError("special_z_classes must lie in [0, 32), got %r" % (special,))
    r = V.TrainRule()
    for k in ("bldg_ins_min", "bldg_ins_max", "car_ins_min", "car_ins_max", "facade_class", "roof_class", "car_class"):
        setattr(r, k, int(getattr(rule, k)))
    r.n_classes = n
    r.special_z_classes = sum(1 << c for c in set(special))
    r.scale_factor, r.proj_size = float(rule.scale_factor), float(rule.proj_size)
    return r


# ---- the workspace -------------------------------------------------------------------------------------------------------
class Workspace:
    """The library's workspace for one device, zero-filled once: the emit leaves its counters zero again and the count
    clears what it uses, so it serves call after call on one stream.  `flag` is the word the emit stores the number of
    flagged rows in -- a 0-d int32 view, rewritten by the next call."""

    def __init__(self, device):
        self.device = torch.device(device)
        nbytes = V.lib().gcv_train_inputs_workspace_bytes(0)
        if nbytes == 0:
            V.check(-1, "gcv_train_inputs_workspace_bytes")
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        o = V.TRAIN_INPUTS_FLAG_OFFSET
        self.flag = self.buf[o:o + 4].view(torch.int32).reshape(())


_default_ws = {}  # (device, stream) -> Workspace, for the calls that bring none


def _workspace(workspace, dev):
    if workspace is None:
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        workspace = _default_ws.get(key)
        if workspace is None:
            workspace = _default_ws[key] = Workspace(dev)
    if workspace.device != dev:
        raise RuntimeError("the workspace lives on %s, pts on %s" % (workspace.device, dev))
    return workspace


# ---- the operator --------------------------------------------------------------------------------------------------------
TrainInputs = collections.namedtuple("TrainInputs", "abs_xyz rel_xyz bch_idx instances classes scales onehots z proj_uv flag")
TrainInputs.__doc__ = """core/train.py:207-224's names: abs_xyz [B,N,3], rel_xyz [B,N,3] and instances [B,N,1] (views of pts),
bch_idx int64 [B,N], classes [B,N,1], scales [B,N,3], onehots [B,N,n_classes], z (None or a model_inputs.GroupedCodes),
proj_uv [B,N,2]; flag: 0-d int32 on the device, the number of flagged rows (an instance that is no integer in [0, 32768)
or a class outside [0, n_classes)) -- a view of the workspace's word, rewritten by the next call on that workspace."""


def _ptr(t):
    return None if t is None else t.data_ptr()


def _tlp(proj_tlp, b, dev):
    """proj_tlp as float32 [B,2] on the device, converted on its own side and never read back: torch promotes an integer
    tensor against the float32 coordinates to float32.  A float64 tensor would promote proj_uv to float64 upstream: refused."""
    if proj_tlp is None:
        return None
    t = torch.as_tensor(proj_tlp)
    if t.dtype == torch.float64:
        raise TypeError("a float64 proj_tlp promotes proj_uv to float64 upstream; pass integers or float32")
    if t.numel() != 2 * b:
        raise ValueError("proj_tlp must hold two values (x, y) per batch element: %d, got %d" % (2 * b, t.numel()))
    if t.is_cuda and t.device != dev:
        raise RuntimeError("proj_tlp lives on %s, pts on %s" % (t.device, dev))
    t = t.to(torch.float32).reshape(b, 2)
    return _dense(t if t.is_cuda else t.to(dev), 4)


def _rows(pts):
    """pts as the library reads it: (tensor holding the memory, row stride in elements).  A view whose last stride is 1,
    whose row stride is at least 9 and whose batch stride is N row strides is taken as it is."""
    b, n, _ = pts.shape
    if pts.stride(2) == 1 and pts.stride(1) >= 9 and (b == 1 or pts.stride(0) == n * pts.stride(1)) and pts.data_ptr() % 4 == 0:
        return pts, pts.stride(1)
    return _dense(pts, 4), 9


def _codes(L, mem, stride, n, ws, z_dim, dev, rule=None, tlp=None, outs=(None,) * 5):
    """count (the wait), emit with groups, then the I draws and their one copy -> GroupedCodes."""
    z_dim = int(z_dim)
    nbytes = ws.buf.numel()
    counts = (C.c_int64 * 2)()
    V.check(L.gcv_train_inputs_count(mem.data_ptr(), stride, n, ws.buf.data_ptr(), nbytes, counts, _stream()),
            "gcv_train_inputs_count")
    n_ins = int(counts[0])
    group = torch.empty((n,), dtype=torch.int32, device=dev)
    ids = torch.empty((n_ins,), dtype=torch.int16, device=dev)
    if rule is None:  # get_z: the groups alone -- every id is class 0 of a one-hot of one, so only the id can flag a row
        rule = V.TrainRule(bldg_ins_min=0, bldg_ins_max=32768, n_classes=1, proj_size=1.0)
    V.check(L.gcv_train_inputs_emit(mem.data_ptr(), stride, n, n, C.byref(rule), _ptr(tlp), ws.buf.data_ptr(), nbytes, 1, n_ins,
                                    *outs, group.data_ptr(), ids.data_ptr() if n_ins else None, _stream()),
            "gcv_train_inputs_emit")
    if n_ins:
        host = torch.empty((n_ins, z_dim), dtype=torch.float32, pin_memory=True)
        for g in range(n_ins):  # utils/helpers.py:144-146: one draw per instance, ascending (one randn(I, z_dim) differs)
            host[g:g + 1].copy_(torch.randn(1, z_dim))
        codes = host.to(dev, non_blocking=True)
    else:
        codes = torch.empty((0, z_dim), dtype=torch.float32, device=dev)
    return GroupedCodes(group, codes, ids)


def prepare(pts, rule, z_dim=None, proj_tlp=None, workspace=None, check=False):
    """core/train.py:207-224 on the device.  pts: float32 CUDA [B,N,9] rows (x, y, z, scale, instance, rel_x, rel_y,
    rel_z, batch); rule: a TrainRule; z_dim: None (z is None; one launch, no host wait) or cfg.NETWORK.GAUSSIAN.Z_DIM
    (B must be 1; one count -- the only wait -- one launch and one asynchronous copy of the codes); proj_tlp: None, a
    host array or tensor, or a device tensor [B,2] of an integer or float32 dtype; workspace: a Workspace kept by the
    caller (default: one per device and stream, kept here); check: wait and raise ValueError on a flagged row."""
    if not isinstance(pts, torch.Tensor) or not pts.is_cuda:
        raise RuntimeError("prepare expects pts on the GPU (the product has no CPU path)")
    if pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[2] != 9:
        raise TypeError("pts must be float32 [B, N, 9], got %s %s" % (pts.dtype, tuple(pts.shape)))
    dev = pts.device
    b, n, _ = pts.shape
    if z_dim is not None:
        assert b == 1, "Unexpected tensor shape (%d, %d, %d)" % (b, n, 1)  # get_z's own assertion
    native = _native_rule(rule)
    nc = int(native.n_classes)
    abs_xyz, rel_xyz, instances = pts[:, :, :3], pts[:, :, 5:8], pts[:, :, 4:5]
    e = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    bch_idx, classes, scales, onehots, proj_uv = e((b, n), torch.int64), e((b, n, 1)), e((b, n, 3)), e((b, n, nc)), e((b, n, 2))
    _STATS["prepare_calls"] += 1
    if b * n == 0:
        z = None if z_dim is None else GroupedCodes(e((0,), torch.int32), e((0, int(z_dim))), e((0,), torch.int16))
        return TrainInputs(abs_xyz, rel_xyz, bch_idx, instances, classes, scales, onehots, z, proj_uv,
                           torch.zeros((), dtype=torch.int32, device=dev))
    tlp = _tlp(proj_tlp, b, dev)
    mem, stride = _rows(pts)
    L = V.lib()
    with torch.cuda.device(dev):
        ws = _workspace(workspace, dev)
        outs = (classes.data_ptr(), scales.data_ptr(), onehots.data_ptr(), proj_uv.data_ptr(), bch_idx.data_ptr())
        if z_dim is None:
            z = None
            V.check(L.gcv_train_inputs_emit(mem.data_ptr(), stride, b * n, n, C.byref(native), _ptr(tlp), ws.buf.data_ptr(),
                                            ws.buf.numel(), 0, 0, *outs, None, None, _stream()), "gcv_train_inputs_emit")
        else:
            z = _codes(L, mem, stride, n, ws, z_dim, dev, native, tlp, outs)
    if check:
        flagged = int(ws.flag.item())
        if flagged:
            raise ValueError("%d row(s) whose instance is not an integer in [0, 32768) or whose class is outside [0, %d)"
                             % (flagged, nc))
    return TrainInputs(abs_xyz, rel_xyz, bch_idx, instances, classes, scales, onehots, z, proj_uv, ws.flag)


def get_z(instances, z_dim):
    """utils.helpers.get_z for a CUDA float32 [1,N,1]: a GroupedCodes that yields upstream's {"z", "idx"} entries, the
    codes upstream's draws in upstream's order.  One host wait (the count) instead of one per instance."""
    if z_dim is None:
        return None
    if not isinstance(instances, torch.Tensor) or not instances.is_cuda:
        raise RuntimeError("get_z expects instances on the GPU (the product has no CPU path)")
    b, n, c = instances.size()
    assert b == 1 and c == 1, "Unexpected tensor shape (%d, %d, %d)" % (b, n, c)
    if instances.dtype != torch.float32:
        raise TypeError("instances must be float32, got %s" % instances.dtype)
    dev = instances.device
    _STATS["get_z_calls"] += 1
    if n == 0:
        return GroupedCodes(torch.empty((0,), dtype=torch.int32, device=dev),
                            torch.empty((0, int(z_dim)), dtype=torch.float32, device=dev),
                            torch.empty((0,), dtype=torch.int16, device=dev))
    rows = torch.empty((n, 9), dtype=torch.float32, device=dev)  # the library reads column 4 alone for the groups
    rows[:, 4] = instances.reshape(n)
    with torch.cuda.device(dev):
        return _codes(V.lib(), rows, 9, n, _workspace(None, dev), z_dim, dev)


def install(helpers_module):
    """Rebinds helpers_module.get_z (utils.helpers of a GaussianCity checkout) to get_z above, for callers who keep
    train.py's lines.  A CPU tensor goes to the function bound before."""
    if hasattr(helpers_module, _ORIGINAL):
        return
    original = helpers_module.get_z

    def installed_get_z(instances, z_dim):
        if z_dim is None or not getattr(instances, "is_cuda", False):
            return original(instances, z_dim)
        return get_z(instances, z_dim)

    setattr(helpers_module, _ORIGINAL, original)
    helpers_module.get_z = installed_get_z


def uninstall(helpers_module):
    original = getattr(helpers_module, _ORIGINAL, None)
    if original is not None:
        helpers_module.get_z = original
        delattr(helpers_module, _ORIGINAL)
