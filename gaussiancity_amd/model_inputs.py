"""Per-model generator inputs and the [N,14] Gaussian tensor on the device, over libgcv_hip.so (include/gcv.h K17, K18;
DESIGN.md section 13b): what scripts/inference.py:239-256 does on the host between the visible point set and the
rasterizer -- three torch.isin masks, per model five boolean-mask gathers, torch.unique and a Python renumbering loop, _get_z
with one host wait, one host-to-device copy and one M-element mask per visible instance, get_one_hot, get_projection_uv,
a torch.cat per key and get_gaussian_points -- as one count (the only host wait), one emit and one assembly launch.

  StyleTable / style_table(style_lut, device)   upstream's {instance: [1, z_dim]} dict as a device table, built once
  MODEL_RULE_GOOGLE_EARTH / MODEL_RULE_KITTI_360   class -> model slot (BLDG, CAR, REST in upstream's dict order)
  split_by_model(visible_set, rule, ...)        ModelSplit: per present model a ModelInputs with what
                                                _get_gaussian_attributes hands the generator
  GroupedCodes                                  the `zs` of a model: group vector + code table, a read-only mapping that
                                                still yields _get_z's {"z", "idx"} entries to code that asks for them
  gaussian_points14(split, attrs_per_model)     [1,N,14] from the generators' outputs in one launch
  stats() / reset_stats()

torch supplies device memory and the current stream; every computation is in the HIP library.  There is no CPU path.
"""
import collections
import collections.abc
import ctypes as C

import torch

from . import _native_v as V
from ._loader import current_stream as _stream
from ._loader import dense as _dense

MODELS = ("BLDG", "CAR", "REST")  # the key order of upstream's `models` dict (scripts/inference.py:470)
_STATS = {"split_calls": 0, "points14_calls": 0}


def stats():
    """Counters of this process: calls of split_by_model and of gaussian_points14."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


# ---- the rule: which model a class belongs to ------------------------------------------------------------------------
ModelRule = collections.namedtuple("ModelRule", "n_classes model_of_class")
ModelRule.__doc__ = """n_classes: the one-hot's width (1..32).  model_of_class: per class 0, 1, 2 = the slot of BLDG, CAR, REST,
or -1: rows of that class are dropped (upstream skips a model that is None)."""


def _rule(class_rule, n_classes, bldg, car, rest):
    table = [2 if rest else -1] * n_classes
    if bldg:  # _get_pt_indexes_by_models: an absent model's classes stay with REST
        table[class_rule.facade_class] = table[class_rule.roof_class] = 0
    if car and class_rule.car_ins_min > 0:
        table[class_rule.car_class] = 1
    return ModelRule(n_classes, tuple(table))


def MODEL_RULE_GOOGLE_EARTH(bldg=True, rest=True):
    """GOOGLE_EARTH (N_CLASSES 8, no CAR class): BLDG_FACADE and BLDG_ROOF to BLDG when that model exists."""
    from . import points
    return _rule(points.CLASS_RULE_GOOGLE_EARTH, 8, bldg, False, rest)


def MODEL_RULE_KITTI_360(bldg=True, car=True, rest=True):
    """KITTI_360 (N_CLASSES 8): BLDG_FACADE and BLDG_ROOF to BLDG, CAR to CAR, when those models exist."""
    from . import points
    return _rule(points.CLASS_RULE_KITTI_360, 8, bldg, car, rest)


def _as_f32_pair(proj_tlp):
    """proj_tlp as the float32 pair `xyz[..., :2] - proj_tlp.unsqueeze(1)` uses: torch promotes an integer tensor against
    the float32 coordinates to float32.  A float64 array would promote the difference to float64 upstream: refused."""
    if proj_tlp is None:
        return 0.0, 0.0
    t = torch.as_tensor(proj_tlp).reshape(-1)
    if t.numel() != 2:
        raise ValueError("proj_tlp must hold two values (x, y), got %d" % t.numel())
    if t.dtype == torch.float64:
        raise TypeError("a float64 proj_tlp promotes proj_uv to float64 upstream; pass integers or float32")
    x, y = t.to(torch.float32).tolist()
    return x, y


def _native_rule(rule, proj_tlp, proj_size):
    n = int(rule.n_classes)
    if not 1 <= n <= 32 or len(rule.model_of_class) < n:
        raise ValueError("n_classes must be in [1, 32] and model_of_class hold a slot per class")
    if any(int(m) not in (-1, 0, 1, 2) for m in rule.model_of_class[:n]):
        raise ValueError("model_of_class must hold -1, 0, 1 or 2")
    r = V.ModelRule()
    r.n_classes = n
    for c in range(32):
        r.model_of_class[c] = int(rule.model_of_class[c]) if c < n else -1
    r.proj_tlp[0], r.proj_tlp[1] = _as_f32_pair(proj_tlp)
    r.proj_size = float(proj_size)
    return r


# ---- the style LUT -----------------------------------------------------------------------------------------------------
class StyleTable:
    """Upstream's style_lut {instance: [1, z_dim] tensor} (scripts/inference.py:136-156) as what gcv_model_split_* read:
    lut float32 [n_lut, z_dim] (row i = instance i) and lut_has uint8 [n_lut] (1 = the dict has i), on `device`."""

    def __init__(self, style_lut, device):
        keys = [int(k) for k in style_lut]
        if any(k < 0 or k > 32767 for k in keys):
            raise KeyError("instance ids are int16 and not negative: %r" % [k for k in keys if k < 0 or k > 32767][:4])
        widths = {int(v.numel()) for v in style_lut.values()}
        if len(widths) > 1:
            raise ValueError("style codes must have one width, got %s" % sorted(widths))
        self.z_dim = widths.pop() if widths else 0
        self.n_lut = max(keys) + 1 if keys else 0
        lut = torch.zeros((self.n_lut, self.z_dim), dtype=torch.float32)
        has = torch.zeros((self.n_lut,), dtype=torch.uint8)
        for k, v in style_lut.items():
            lut[int(k)] = v.detach().reshape(-1).to(dtype=torch.float32, device="cpu")
            has[int(k)] = 1
        self.device = torch.device(device)
        self.lut, self.lut_has = lut.to(self.device), has.to(self.device)


_style_cache = {}  # id(dict) -> [len(dict), {device: StyleTable}]


def style_table(style_lut, device):
    """The StyleTable of a dict, built once per dict and device and kept (keyed on the dict's id and length, as
    points.centers_table: a dict that grew or shrank is converted again)."""
    e = _style_cache.get(id(style_lut))
    if e is None or e[0] != len(style_lut):
        e = _style_cache[id(style_lut)] = [len(style_lut), {}]
    device = torch.device(device)
    if device not in e[1]:
        e[1][device] = StyleTable(style_lut, device)
    return e[1][device]


_cached_style_table = style_table  # (split_by_model has a parameter of that name)


# ---- zs ------------------------------------------------------------------------------------------------------------------
class GroupedCodes(collections.abc.Mapping):
    """The style codes of one model's rows: `group` int32 [n] (the rank of a row's instance among the model's instances
    that have a code, -1: none), `codes` float32 [G, z_dim] and `instances` int16 [G] (ascending).  It stands for the dict
    _get_z returns, {instance: {"z": [1, z_dim], "idx": bool [1, n]}} in ascending instance order, and yields those
    entries -- the masks made on the spot -- to code that asks for them (GaussianAttrMLP.forward uses `zs is None` and
    `zs.values()`).  attr_head and attr_chain read `group` and `codes` directly.  Read-only, and not a dict: it passes
    through torch.nn.DataParallel's scatter as the same object."""
    __slots__ = ("group", "codes", "instances", "_keys")

    def __init__(self, group, codes, instances):
        object.__setattr__(self, "group", group)
        object.__setattr__(self, "codes", codes)
        object.__setattr__(self, "instances", instances)
        object.__setattr__(self, "_keys", None)

    def __setattr__(self, name, value):
        raise TypeError("GroupedCodes is read-only")

    def __delattr__(self, name):
        raise TypeError("GroupedCodes is read-only")

    def __len__(self):
        return int(self.codes.shape[0])

    def _entry(self, g):
        return {"z": self.codes[g:g + 1], "idx": (self.group == g).unsqueeze(0)}

    def _ids(self):
        if self._keys is None:  # the only host copy, and only for code that wants the ids
            object.__setattr__(self, "_keys", tuple(int(i) for i in self.instances.tolist()))
        return self._keys

    def __iter__(self):
        return iter(self._ids())

    def __getitem__(self, instance):
        try:
            return self._entry(self._ids().index(instance))
        except ValueError:
            raise KeyError(instance) from None

    def __contains__(self, instance):
        return instance in self._ids()

    def keys(self):
        return list(self._ids())

    def values(self):
        return [self._entry(g) for g in range(len(self))]

    def items(self):
        return list(zip(self._ids(), self.values()))

    def __repr__(self):
        return "GroupedCodes(n=%d, G=%d, z_dim=%d)" % (self.group.shape[0], self.codes.shape[0], self.codes.shape[1])


# ---- the split -------------------------------------------------------------------------------------------------------
ModelInputs = collections.namedtuple("ModelInputs", "abs_xyz rel_xyz batch_idx onehots proj_uv classes scales zs index")
ModelInputs.__doc__ = """One model's rows: abs_xyz [1,n,3] and rel_xyz [1,n,3] (views of the split's pts), batch_idx int32 [1,n],
onehots [1,n,n_classes], proj_uv [1,n,2] -- the generator's arguments -- and classes [1,n,1], scales [1,n,3],
zs (None or GroupedCodes), index int64 [n] (positions in the visible set)."""
ModelSplit = collections.namedtuple("ModelSplit", "models pts abs_xyz scales index counts")
ModelSplit.__doc__ = """models: {name: ModelInputs} for the models that have rows, in upstream's order; pts [1,N,8], abs_xyz
[1,N,3] (a view of pts) and scales [1,N,3]: the models' rows one after the other, as _get_pt_attrs_by_models concatenates
them; index int64 [N]; counts: {name: (rows, instances, instances with a code)}."""


def _ptr(t):
    return None if t is None else t.data_ptr()


def split_by_model(visible_set, model_rule, style_table=None, proj_tlp=None, proj_size=2048, workspace=None):
    """scripts/inference.py:239-253 up to the generator calls, on the device.  visible_set: points.VisibleSet; model_rule:
    a ModelRule; style_table: a StyleTable, upstream's style_lut dict, or None (no style codes); proj_tlp: None or the
    two values of local_projections["tlp"] (host values: they travel in the kernel's arguments); proj_size: PROJ_SIZE;
    workspace: a points.VisibleSetWorkspace of its own, kept across frames (every count clears what it uses).
    One host wait (the counts)."""
    pts, batch_idx, instances = visible_set.pts, visible_set.batch_idx, visible_set.instances
    classes, scales = visible_set.classes, visible_set.scales
    dev = pts.device
    if dev.type != "cuda":
        raise RuntimeError("split_by_model expects a visible set on the GPU (the product has no CPU path)")
    m, k = int(pts.shape[1]), int(instances.numel())
    checks = ((pts, torch.float32, (1, m, 8)), (batch_idx, torch.int32, (1, m, 1)), (classes, torch.float32, (1, m, 1)),
              (scales, torch.float32, (1, m, 3)), (instances, torch.int16, (k,)))
    for t, dt, shape in checks:
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev:
            raise TypeError("visible_set must hold pts float32 [1,M,8], batch_idx int32 [1,M,1], instances int16 [K], "
                            "classes float32 [1,M,1] and scales float32 [1,M,3] on one device")
    batch_idx, instances, classes, scales = (t.contiguous() for t in (batch_idx, instances, classes, scales))
    pts = _dense(pts)  # the emit reads a row of pts as two 16-byte pieces
    if isinstance(style_table, dict):
        style_table = _cached_style_table(style_table, dev)
    if style_table is not None and style_table.device != dev:
        raise RuntimeError("the style table lives on %s, the visible set on %s" % (style_table.device, dev))
    n_lut = style_table.n_lut if style_table is not None else 0
    z_dim = style_table.z_dim if style_table is not None else 0
    lut, lut_has = (style_table.lut, style_table.lut_has) if n_lut else (None, None)
    rule = _native_rule(model_rule, proj_tlp, proj_size)
    nc = int(rule.n_classes)
    L = V.lib()
    with torch.cuda.device(dev):
        nbytes = L.gcv_model_split_workspace_bytes(m, k)
        if nbytes == 0:
            V.check(-1, "gcv_model_split_workspace_bytes")
        ws = workspace.take(nbytes) if workspace is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = (C.c_int64 * 9)()
        V.check(L.gcv_model_split_count(classes.data_ptr(), batch_idx.data_ptr(), m, _ptr(instances), k, _ptr(lut_has), n_lut,
                                        C.byref(rule), ws.data_ptr(), nbytes, counts, _stream()), "gcv_model_split_count")
        n_m, b_m, g_m = list(counts[0:3]), list(counts[3:6]), list(counts[6:9])
        n, g = sum(n_m), sum(g_m)
        e = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        index, out_pts, batch = e((n,), torch.int64), e((1, n, 8)), e((1, n), torch.int32)
        out_classes, out_scales, onehots, proj_uv = e((1, n, 1)), e((1, n, 3)), e((1, n, nc)), e((1, n, 2))
        group = e((n,), torch.int32) if g else None
        group_instances = e((g,), torch.int16) if g else None
        codes = e((g, z_dim)) if g else None
        V.check(L.gcv_model_split_emit(
            classes.data_ptr(), batch_idx.data_ptr(), pts.data_ptr(), scales.data_ptr(), m, _ptr(instances), k, _ptr(lut_has),
            _ptr(lut), n_lut, z_dim, C.byref(rule), ws.data_ptr(), nbytes, counts, index.data_ptr(), out_pts.data_ptr(),
            batch.data_ptr(), out_classes.data_ptr(), out_scales.data_ptr(), onehots.data_ptr(), proj_uv.data_ptr(),
            _ptr(group), _ptr(group_instances), _ptr(codes), _stream()), "gcv_model_split_emit")
    models, o, go = collections.OrderedDict(), 0, 0
    for name, nm, bm, gm in zip(MODELS, n_m, b_m, g_m):
        if nm:  # upstream skips a model without rows
            s = slice(o, o + nm)
            zs = GroupedCodes(group[s], codes[go:go + gm], group_instances[go:go + gm]) if gm else None
            models[name] = ModelInputs(out_pts[:, s, :3], out_pts[:, s, 5:8], batch[:, s], onehots[:, s], proj_uv[:, s],
                                       out_classes[:, s], out_scales[:, s], zs, index[s])
        o, go = o + nm, go + gm
    _STATS["split_calls"] += 1
    return ModelSplit(models, out_pts, out_pts[:, :, :3], out_scales, index,
                      {name: (nm, bm, gm) for name, nm, bm, gm in zip(MODELS, n_m, b_m, g_m)})


# ---- [1,N,14] ------------------------------------------------------------------------------------------------------------
_WIDTH = {"rgb": 3, "xyz": 3, "scale": 3, "opacity": 1}


def gaussian_points14(split, attrs_per_model):
    """utils/helpers.py:226-247 on the per-key concatenation of the models' attribute dicts (scripts/inference.py:495-501)
    in one launch: [1,N,14] = xyz + attrs["xyz"], opacity (1 where absent), scales * attrs["scale"], rotation (1,0,0,0), rgb.
    attrs_per_model: {model name: the generator's output dict} for exactly split.models' names, or a sequence in their
    order.  Neither split.abs_xyz nor split.scales is changed (upstream updates its copies in place).  Inference only."""
    names = list(split.models)
    if isinstance(attrs_per_model, collections.abc.Mapping):
        if set(attrs_per_model) != set(names):
            raise ValueError("attributes for models %s, the split has %s" % (sorted(attrs_per_model), names))
        per = [attrs_per_model[k] for k in names]
    else:
        per = list(attrs_per_model)
        if len(per) != len(names):
            raise ValueError("%d attribute dicts for %d models" % (len(per), len(names)))
    keys = set(per[0]) if per else {"rgb"}
    if any(set(a) != keys for a in per):
        raise ValueError("the models' attribute dicts must have the same keys, got %s" % [sorted(a) for a in per])
    if "rgb" not in keys:
        raise ValueError("the attribute dicts have no 'rgb'")
    pts, scales = split.pts, split.scales
    dev, n = pts.device, int(pts.shape[1])
    rec, keep = V.GaussianAttrs(), []
    rec.n_segments = max(1, len(per))
    for i, (name, a) in enumerate(zip(names, per)):
        nm = int(split.models[name].index.shape[0])
        rec.seg[i].n = nm
        for key, field in (("rgb", "rgb"), ("xyz", "dxyz"), ("scale", "scale"), ("opacity", "opacity")):
            if key not in a:
                continue
            t = a[key]
            if not t.is_cuda or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != (1, nm, _WIDTH[key]):
                raise TypeError("%s of %s must be a float32 CUDA tensor [1, %d, %d]" % (key, name, nm, _WIDTH[key]))
            t = t.detach().contiguous()
            keep.append(t)
            setattr(rec.seg[i], field, t.data_ptr())
    out = torch.empty((1, n, 14), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        V.check(V.lib().gcv_gaussian_points(pts.data_ptr(), 8, scales.data_ptr(), 3, n, rec, out.data_ptr(), _stream()), "gcv_gaussian_points")
    _STATS["points14_calls"] += 1
    return out
