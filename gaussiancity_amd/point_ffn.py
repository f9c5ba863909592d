"""The feed-forward third of the PTv3 point backbone's Block over libgcm_hip.so (include/gcm.h):
Block.forward ends with LayerNorm, Linear(C, 4C), GELU, Linear(4C, C), DropPath and the residual add -- five launches
and the [N, 4C] tensor through memory twice; install() rebinds the method so that this tail is one call of
ffn.layernorm_mlp_residual.

  install(pt_v3, max_channels=None, split=False) / uninstall(pt_v3)
                                        rebind Block.forward of a caller's imported models.pt_v3
  stats() / reset_stats()               calls that took the fused tail, calls that went to the module's own method
  split_stats()                         the fused tails that ran the split entry points (ffn.layernorm_mlp_residual's split=True)

max_channels=None keeps the width ffn.max_channels() holds; an int up to ffn.split_max_channels() sends the wider Blocks it
admits through the split entry points, and split=True the narrower ones as well (the same bits: the choice is speed alone).

The rebound method runs cpe, the first residual, norm1, attn and drop_path through the modules themselves, so
point_attention, point_index, point_pool and the sparse drop-ins keep composing, and the first DropPath mask is drawn
first, as upstream.  post-norm Blocks, other norm or activation layers, a tanh GELU, CPU tensors, other dtypes, an active
autocast and widths the library does not hold go to the module's own method, untouched.

fused_tail(point, parts) is the tail alone, for point_front, whose rebound method runs it after its own front; installed over
point_front's method, this one hands it the Blocks it accepts (point_front.py).
"""
import torch

from . import ffn

_STATS = {"fused_calls": 0, "original_calls": 0}
_SPLIT_STATS = {"fused_calls": 0}
_ORIGINAL = "_gaussiancity_amd_point_ffn_original"
_CAP = "_gaussiancity_amd_point_ffn_max_channels"
_SPLIT = "_gaussiancity_amd_point_ffn_split"


def stats():
    """Counters of this process: forwards whose tail ran the fused kernels, forwards handed to the module's own method."""
    return dict(_STATS)


def split_stats():
    """The fused calls among stats() whose tail ran the split entry points."""
    return dict(_SPLIT_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0
    _SPLIT_STATS["fused_calls"] = 0


def _limit(pt_v3_module):
    """The widest Block install() admitted on this module: the one-launch kernels' limit without a cap."""
    cap = getattr(pt_v3_module, _CAP, None) if pt_v3_module is not None else None
    return ffn.max_channels() if cap is None else cap


def takes_split(pt_v3_module, C):
    """Whether a Block of width C that _parts accepted runs the split entry points on this module."""
    return C > ffn.max_channels() or bool(getattr(pt_v3_module, _SPLIT, False))


def _only(container):
    """The one sub-module of a PointSequential, or None."""
    mods = list(getattr(container, "_modules", {}).values())
    return mods[0] if len(mods) == 1 else None


def _parts(self, point, pt_v3_module=None):
    """(LayerNorm, MLP, DropPath or None) when the Block's tail is what the operator computes, else None.  pt_v3_module:
    the module install() was called on, whose max_channels admits wider Blocks; without it the one-launch kernels' limit."""
    if not getattr(self, "pre_norm", False):
        return None
    norm, mlp, drop = _only(self.norm2), _only(self.mlp), _only(self.drop_path)
    if type(norm) is not torch.nn.LayerNorm or norm.weight is None or norm.bias is None or len(norm.normalized_shape) != 1:
        return None
    fc1, act, fc2 = (getattr(mlp, n, None) for n in ("fc1", "act", "fc2"))
    if not isinstance(fc1, torch.nn.Linear) or not isinstance(fc2, torch.nn.Linear) or fc1.bias is None or fc2.bias is None:
        return None
    if type(act) is not torch.nn.GELU or act.approximate != "none":
        return None
    if isinstance(drop, torch.nn.Identity):
        drop = None
    elif drop is None or not hasattr(drop, "drop_prob") or not hasattr(drop, "scale_by_keep"):
        return None
    feat = point.feat
    if not feat.is_cuda or feat.dtype != torch.float32 or feat.dim() != 2 or torch.is_autocast_enabled():
        return None
    C, Hd = feat.shape[1], fc1.out_features
    if norm.normalized_shape[0] != C or fc1.in_features != C or fc2.in_features != Hd or fc2.out_features != C:
        return None
    hidden = 4 * (ffn.split_max_channels() if takes_split(pt_v3_module, C) else ffn.max_channels())
    if C % 4 or Hd % 4 or C > _limit(pt_v3_module) or Hd > hidden:
        return None
    return norm, mlp, drop


def fused_tail(point, parts, split=False):
    """Block.forward's last third on point.feat (the tail's shortcut) over ffn.layernorm_mlp_residual; parts is what
    _parts accepted, split what takes_split says.  Sets point.feat and point.sparse_conv_feat as the method does; counted
    as a fused call."""
    norm, mlp, drop = parts
    feat, row_scale = point.feat, None
    if drop is not None and drop.drop_prob and drop.training:  # DropPath._drop_path's mask, drawn as it draws it
        keep = 1 - drop.drop_prob
        row_scale = feat.new_empty((feat.shape[0], 1)).bernoulli_(keep)
        if keep > 0.0 and drop.scale_by_keep:
            row_scale.div_(keep)
    point.feat = ffn.layernorm_mlp_residual(feat, norm.weight, norm.bias, norm.eps, mlp.fc1.weight, mlp.fc1.bias,
                                            mlp.fc2.weight, mlp.fc2.bias, row_scale, split=split)
    point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
    _STATS["fused_calls"] += 1
    if split:
        _SPLIT_STATS["fused_calls"] += 1
    return point


# ---- the method of models/pt_v3.py, written against its behaviour: the order of its modules, of its residual adds and of
# the DropPath draws, and the attributes it sets on the point ---------------------------------------------------------------
def _forward(original, pt_v3_module):
    def forward(self, point):
        """Block.forward (pre_norm) with its last third over ffn.layernorm_mlp_residual."""
        front_accepts = getattr(original, "block_front_accepts", None)
        if front_accepts is not None and front_accepts(self, point):
            return original(self, point)  # point_front's method, bound before this one: it runs this tail itself
        parts = _parts(self, point, pt_v3_module)
        if parts is None:
            _STATS["original_calls"] += 1
            return original(self, point)
        shortcut = point.feat
        point = self.cpe(point)
        point.feat = shortcut + point.feat
        shortcut = point.feat
        point = self.norm1(point)
        point = self.drop_path(self.attn(point))
        point.feat = shortcut + point.feat
        return fused_tail(point, parts, takes_split(pt_v3_module, point.feat.shape[1]))
    return forward


def install(pt_v3_module, max_channels=None, split=False):
    """Rebind Block.forward of the caller's imported models.pt_v3 so that its feed-forward tail runs the fused kernels.
    max_channels: None for the widths the one-launch kernels hold, or an int up to ffn.split_max_channels(): Blocks wider
    than ffn.max_channels() and no wider than it run the split entry points.  split=True sends the narrower Blocks
    through them too.  Idempotent (new keyword values are taken over); uninstall() puts the module's own method back."""
    if max_channels is not None and (not isinstance(max_channels, int) or isinstance(max_channels, bool) or max_channels < 0):
        raise ValueError("max_channels must be None or a non-negative int, got %r" % (max_channels,))
    if not isinstance(split, bool):
        raise ValueError("split must be a bool, got %r" % (split,))
    if max_channels is not None and max_channels > ffn.split_max_channels():
        raise ValueError("max_channels = %d: the split kernels hold C up to %d" % (max_channels, ffn.split_max_channels()))
    ffn.max_channels()  # loads the library: a build without the operator fails here, not inside a forward
    setattr(pt_v3_module, _CAP, max_channels)
    setattr(pt_v3_module, _SPLIT, split)
    if getattr(pt_v3_module, _ORIGINAL, None) is not None:
        return
    original = pt_v3_module.Block.forward
    setattr(pt_v3_module, _ORIGINAL, original)
    pt_v3_module.Block.forward = _forward(original, pt_v3_module)


def uninstall(pt_v3_module):
    original = getattr(pt_v3_module, _ORIGINAL, None)
    if original is None:
        return
    pt_v3_module.Block.forward = original
    for name in (_ORIGINAL, _CAP, _SPLIT):
        delattr(pt_v3_module, name)
