"""The feed-forward third of the PTv3 point backbone's Block over libgcm_hip.so (include/gcm.h):
Block.forward ends with LayerNorm, Linear(C, 4C), GELU, Linear(4C, C), DropPath and the residual add -- five launches
and the [N, 4C] tensor through memory twice; install() turns this third on in point_block's rebound method, where the tail is
one call of ffn.layernorm_mlp_residual.

  install(pt_v3, max_channels=None, split=False) / uninstall(pt_v3)
                                        turn the third on / off for a caller's imported models.pt_v3
  stats() / reset_stats()               calls that took the fused tail, calls that went to the module's own method
  split_stats()                         the fused tails that ran the split entry points (ffn.layernorm_mlp_residual's split=True)

max_channels=None keeps the width ffn.max_channels() holds; an int up to ffn.split_max_channels() sends the wider Blocks it
admits through the split entry points, and split=True the narrower ones as well (the same bits: the choice is speed alone).

Without point_front the method runs cpe, the first residual, norm1, attn and drop_path through the modules themselves, so
point_attention, point_index, point_pool and the sparse drop-ins keep composing, and the first DropPath mask is drawn
first, as upstream.  post-norm Blocks, other norm or activation layers, a tanh GELU, CPU tensors, other dtypes, an active
autocast and widths the library does not hold go to the module's own method, untouched.

fused_tail(point, parts) is the tail alone; the rebound method (point_block.py) runs it after upstream's lines or after
point_front's and point_mid's, whichever thirds are on, in any order of the installs.
"""
import torch

from . import ffn, point_block

_STATS = {"fused_calls": 0, "original_calls": 0}
_SPLIT_STATS = {"fused_calls": 0}


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


def _installed(pt_v3_module):
    """(the widest Block, split) as install() set them on this module: the one-launch kernels' limit without it."""
    st = point_block.state(pt_v3_module)
    return (ffn.max_channels(), False) if st is None or st.ffn is None else st.ffn


def takes_split(pt_v3_module, C):
    """Whether a Block of width C that _parts accepted runs the split entry points on this module."""
    return C > ffn.max_channels() or _installed(pt_v3_module)[1]


def _only(container):
    """The one sub-module of a PointSequential, or None."""
    mods = list(getattr(container, "_modules", {}).values())
    return mods[0] if len(mods) == 1 else None


def drop_path_of(self):
    """The Block's DropPath: None for an Identity, False for what is neither an Identity nor DropPath-like."""
    drop = _only(self.drop_path)
    if isinstance(drop, torch.nn.Identity):
        return None
    return drop if hasattr(drop, "drop_prob") and hasattr(drop, "scale_by_keep") else False


def row_scale(drop, feat):
    """DropPath._drop_path's mask for the rows of feat, drawn as it draws it; None where it draws nothing."""
    if drop is None or not drop.drop_prob or not drop.training:
        return None
    keep = 1 - drop.drop_prob
    mask = feat.new_empty((feat.shape[0], 1)).bernoulli_(keep)
    if keep > 0.0 and drop.scale_by_keep:
        mask.div_(keep)
    return mask


def _parts(self, point, pt_v3_module=None):
    """(LayerNorm, MLP, DropPath or None) when the Block's tail is what the operator computes, else None.  pt_v3_module:
    the module install() was called on, whose max_channels admits wider Blocks; without it the one-launch kernels' limit."""
    if not getattr(self, "pre_norm", False):
        return None
    norm, mlp, drop = _only(self.norm2), _only(self.mlp), drop_path_of(self)
    if type(norm) is not torch.nn.LayerNorm or norm.weight is None or norm.bias is None or len(norm.normalized_shape) != 1:
        return None
    fc1, act, fc2 = (getattr(mlp, n, None) for n in ("fc1", "act", "fc2"))
    if not isinstance(fc1, torch.nn.Linear) or not isinstance(fc2, torch.nn.Linear) or fc1.bias is None or fc2.bias is None:
        return None
    if type(act) is not torch.nn.GELU or act.approximate != "none":
        return None
    if drop is False:
        return None
    feat = point.feat
    if not feat.is_cuda or feat.dtype != torch.float32 or feat.dim() != 2 or torch.is_autocast_enabled():
        return None
    C, Hd = feat.shape[1], fc1.out_features
    if norm.normalized_shape[0] != C or fc1.in_features != C or fc2.in_features != Hd or fc2.out_features != C:
        return None
    hidden = 4 * (ffn.split_max_channels() if takes_split(pt_v3_module, C) else ffn.max_channels())
    if C % 4 or Hd % 4 or C > _installed(pt_v3_module)[0] or Hd > hidden:
        return None
    return norm, mlp, drop


def fused_tail(point, parts, split=False):
    """Block.forward's last third on point.feat (the tail's shortcut) over ffn.layernorm_mlp_residual; parts is what
    _parts accepted, split what takes_split says.  Sets point.feat and point.sparse_conv_feat as the method does; counted
    as a fused call."""
    norm, mlp, drop = parts
    feat = point.feat
    point.feat = ffn.layernorm_mlp_residual(feat, norm.weight, norm.bias, norm.eps, mlp.fc1.weight, mlp.fc1.bias,
                                            mlp.fc2.weight, mlp.fc2.bias, row_scale(drop, feat), split=split)
    point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
    _STATS["fused_calls"] += 1
    if split:
        _SPLIT_STATS["fused_calls"] += 1
    return point


def install(pt_v3_module, max_channels=None, split=False):
    """Have Block.forward of the caller's imported models.pt_v3 run its feed-forward tail on the fused kernels.
    max_channels: None for the widths the one-launch kernels hold, or an int up to ffn.split_max_channels(): Blocks wider
    than ffn.max_channels() and no wider than it run the split entry points.  split=True sends the narrower Blocks
    through them too.  Idempotent (new keyword values are taken over); uninstall() turns the third off again."""
    if max_channels is not None and (not isinstance(max_channels, int) or isinstance(max_channels, bool) or max_channels < 0):
        raise ValueError("max_channels must be None or a non-negative int, got %r" % (max_channels,))
    if not isinstance(split, bool):
        raise ValueError("split must be a bool, got %r" % (split,))
    if max_channels is not None and max_channels > ffn.split_max_channels():
        raise ValueError("max_channels = %d: the split kernels hold C up to %d" % (max_channels, ffn.split_max_channels()))
    limit = ffn.max_channels()  # loads the library: a build without the operator fails here, not inside a forward
    point_block.turn(pt_v3_module, ffn=(limit if max_channels is None else max_channels, split))


def uninstall(pt_v3_module):
    point_block.turn(pt_v3_module, ffn=None)
