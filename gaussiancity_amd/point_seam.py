"""The seams between the PTv3 point backbone's stages over libgcm_hip.so (include/gcm.h): between
its stages models/pt_v3.py runs the chain Linear -> BatchNorm1d -> GELU as members of a PointSequential -- Embedding.stem's
tail, SerializedUnpooling.proj and proj_skip, and, as two one-module containers, SerializedPooling's norm and act.
install() rebinds PointSequential.forward of a caller's imported models.pt_v3 so that each such run is ONE call of
seam.linear_bn_gelu.

  install(pt_v3) / uninstall(pt_v3)     rebind / restore PointSequential.forward; set / remove the marker point_pool's
                                        rebound SerializedPooling.forward looks for
  pooling_tail(norm, act, point)        point_pool's norm / act tail as one call, when the two containers are that pair
  stats() / reset_stats()               runs fused, pooling tails fused, modules and whole containers run as upstream does

The rebound method walks the container as upstream's does.  Where it meets a run (optional Linear) -> BatchNorm1d ->
(optional GELU(approximate='none')) on a Point it makes one call and leaves point.feat as the run's result;
point.sparse_conv_feat is afterwards exactly what upstream leaves there: the Linear's and the GELU's branch replace its
features, the norm's branch does not, so a run that ends at the norm behind a Linear while the key is present is not fused.
Everything else runs the lines upstream runs for that module, and is counted: other module types (subclasses of the
three among them: their forward is their own), a feature tensor of one
row (upstream skips the norm there) or none, CPU tensors, dtypes other than float32, active autocast, a width beyond
seam.max_channels() or no multiple of 4, affine=False, track_running_stats=False, momentum=None; a container without a
run, and any input that is not a Point, goes to the module's own method whole.

Independent of point_pool, point_front, point_mid and point_ffn: those rebind other methods, in any order.
"""
import torch

from . import seam

_STATS = {"fused_runs": 0, "pooling_tails": 0, "original_modules": 0, "original_calls": 0}
_ORIGINAL = "_gaussiancity_amd_point_seam_original"
_MARK = "_gaussiancity_amd_point_seam_installed"


def stats():
    """Counters of this process: runs that took one fused call (pooling tails among them are also counted on their own),
    modules the rebound walk ran as upstream does, containers handed to the module's own method whole."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _norm_ok(bn, feat):
    """Whether the operator computes this BatchNorm1d on these features."""
    if type(bn) is not torch.nn.BatchNorm1d or not bn.affine or not bn.track_running_stats or bn.momentum is None:
        return False
    if not feat.is_cuda or feat.dtype != torch.float32 or feat.dim() != 2 or feat.shape[0] < 2:
        return False
    if torch.is_autocast_enabled():
        return False
    C = bn.num_features
    return C % 4 == 0 and 0 < C <= seam.max_channels()


def _gelu_ok(module):
    return type(module) is torch.nn.GELU and module.approximate == "none"


def _run_at(mods, i, point):
    """(linear or None, norm, gelu or None, modules taken) for the run that starts at mods[i], or None."""
    linear = mods[i] if type(mods[i]) is torch.nn.Linear else None
    j = i + (linear is not None)
    if j >= len(mods) or not _norm_ok(mods[j], point.feat):
        return None
    bn = mods[j]
    gelu = mods[j + 1] if j + 1 < len(mods) and _gelu_ok(mods[j + 1]) else None
    if linear is not None:
        I, O = linear.in_features, linear.out_features
        if O != bn.num_features or I != point.feat.shape[1] or I % 4 or not 0 < I <= seam.max_channels():
            return None
        if gelu is None and "sparse_conv_feat" in point.keys():  # upstream leaves the Linear's output there
            return None
    elif bn.num_features != point.feat.shape[1]:
        return None
    return linear, bn, gelu, (linear is not None) + 1 + (gelu is not None)


def _call(linear, bn, gelu, feat):
    return seam.linear_bn_gelu(feat, None if linear is None else linear.weight, None if linear is None else linear.bias,
                               bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                               training=bn.training, momentum=bn.momentum, eps=bn.eps, act=gelu is not None)


def _fused_run(run, point):
    linear, bn, gelu, _ = run
    point.feat = _call(linear, bn, gelu, point.feat)
    if (linear is not None or gelu is not None) and "sparse_conv_feat" in point.keys():
        point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
    _STATS["fused_runs"] += 1


# ---- PointSequential.forward's lines for one module, written against their behaviour: a PointModule maps the point, a
# spconv module maps point.sparse_conv_feat and point.feat follows, a BatchNorm1d maps point.feat unless it has one row, any
# other module maps point.feat and the sparse tensor's features follow when the key is present; what is no Point (a
# PointModule may return anything) goes to the module itself, a sparse tensor through its features -------------------------
def _step(module, x, m):
    if isinstance(module, m.PointModule):
        return module(x)
    point = isinstance(x, m.Point)
    if m.spconv.modules.is_spconv_module(module):
        if not point:
            return module(x)
        x.sparse_conv_feat = module(x.sparse_conv_feat)
        x.feat = x.sparse_conv_feat.features
    elif point and isinstance(module, torch.nn.BatchNorm1d):
        if x.feat.size(0) != 1:
            x.feat = module(x.feat)
    elif point:
        x.feat = module(x.feat)
        if "sparse_conv_feat" in x.keys():
            x.sparse_conv_feat = x.sparse_conv_feat.replace_feature(x.feat)
    elif isinstance(x, getattr(m.spconv, "SparseConvTensor", ())):
        if x.indices.shape[0] != 0:
            x = x.replace_feature(module(x.features))
    else:
        x = module(x)
    return x


def _forward(original, m):
    def forward(self, x):
        """PointSequential.forward with every Linear -> BatchNorm1d -> GELU run on a Point as one seam.linear_bn_gelu."""
        mods = list(self._modules.values())
        if not isinstance(x, m.Point) or not any(isinstance(mod, torch.nn.BatchNorm1d) for mod in mods):
            _STATS["original_calls"] += 1
            return original(self, x)
        i = 0
        while i < len(mods):
            run = _run_at(mods, i, x) if isinstance(x, m.Point) else None  # (a PointModule may return something else)
            if run is not None:
                _fused_run(run, x)
                i += run[3]
                continue
            x = _step(mods[i], x, m)
            _STATS["original_modules"] += 1
            i += 1
        return x
    return forward


def pooling_tail(norm, act, point):
    """SerializedPooling's `point = self.norm(point); point = self.act(point)` as one call when norm is a container of one
    BatchNorm1d the operator computes and act a container of one GELU(approximate='none'); True when it ran.  The caller has
    checked that both exist and that the point set has more than one row."""
    n, a = list(getattr(norm, "_modules", {}).values()), list(getattr(act, "_modules", {}).values())
    if len(n) != 1 or len(a) != 1 or not _gelu_ok(a[0]):
        return False
    run = _run_at([n[0], a[0]], 0, point)
    if run is None or run[3] != 2:
        return False
    _fused_run(run, point)
    _STATS["pooling_tails"] += 1
    return True


def install(pt_v3_module):
    """Rebind PointSequential.forward of the caller's imported models.pt_v3 and set the marker for point_pool's pooling
    forward.  Idempotent; uninstall() puts the module's own method back."""
    if getattr(pt_v3_module, _ORIGINAL, None) is not None:
        return
    seam.max_channels()  # loads the library: a build without the operator fails here, not inside a forward
    seq = pt_v3_module.PointSequential
    setattr(pt_v3_module, _ORIGINAL, seq.forward)
    seq.forward = _forward(seq.forward, pt_v3_module)
    setattr(pt_v3_module, _MARK, True)


def uninstall(pt_v3_module):
    original = getattr(pt_v3_module, _ORIGINAL, None)
    if original is None:
        return
    pt_v3_module.PointSequential.forward = original
    delattr(pt_v3_module, _ORIGINAL)
    delattr(pt_v3_module, _MARK)
