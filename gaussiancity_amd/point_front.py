"""The front of the PTv3 point backbone's Block over libgcm_hip.so (include/gcm.h): between its sparse
convolution and its attention Block.forward runs cpe[1] Linear(C, C), cpe[2] LayerNorm(C), the residual add, norm1
LayerNorm(C) and attn.qkv Linear(C, 3C) -- five launches forward and about fourteen backward; install() turns this third on
in point_block's rebound method, where they are one call of front.conv_tail_norm_qkv.

  install(pt_v3, max_channels=None) / uninstall(pt_v3)     turn the third on / off for a caller's imported models.pt_v3
  stats() / reset_stats()               calls that took the fused front, calls the front was on for and turned away

The rebound method (point_block.py) runs the convolution through its module (the sparse drop-ins keep composing), the
attention from the projection on through point_attention.forward_from_qkv (point_attention.install need not have been
called) or point_mid's middle, and the tail through point_ffn's fused tail when point_ffn is on for the same module and
accepts the Block, else through norm2, mlp and drop_path themselves.  The DropPath masks are drawn in upstream's order; the
front draws nothing.  max_channels caps the width that goes to the fused front (narrow Blocks have the rows that fill the
device), the default is the library's limit.  post-norm Blocks, another cpe, other norm layers, an
attention that point_attention does not run, CPU tensors, other dtypes, an active autocast and wider Blocks go to
point_ffn's lines when it takes them, else to the method that was bound before, untouched.

point_front, point_mid and point_ffn go on and come off in any order; none switches another off.
"""
import torch

from . import attention, front, point_attention, point_block, point_ffn

_STATS = {"fused_calls": 0, "original_calls": 0}


def stats():
    """Counters of this process: forwards whose front ran the fused kernels, forwards the front was on for and turned away."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _layer_norm(m, C):
    return type(m) is torch.nn.LayerNorm and m.weight is not None and m.bias is not None and tuple(m.normalized_shape) == (C,)


def _parts(self, point, pt_v3_module):
    """(conv, Linear, LayerNorm, norm1's LayerNorm, attn.qkv) when the Block's front is what the operator computes, else
    None."""
    if not getattr(self, "pre_norm", False):
        return None
    cpe = list(getattr(self.cpe, "_modules", {}).values())
    if len(cpe) != 3 or not pt_v3_module.spconv.modules.is_spconv_module(cpe[0]):
        return None
    conv, lin, lnc = cpe
    ln1, qkv = point_ffn._only(self.norm1), getattr(self.attn, "qkv", None)
    if not isinstance(lin, torch.nn.Linear) or lin.bias is None or not isinstance(qkv, torch.nn.Linear) or qkv.bias is None:
        return None
    feat = point.feat
    if not feat.is_cuda or feat.dtype != torch.float32 or feat.dim() != 2 or torch.is_autocast_enabled():
        return None
    C, O = feat.shape[1], qkv.out_features
    if lin.in_features != C or lin.out_features != C or qkv.in_features != C or not _layer_norm(lnc, C) or not _layer_norm(ln1, C):
        return None
    st = point_block.state(pt_v3_module)
    limit = front.max_channels() if st is None or st.front is None else st.front
    if C % 4 or O % 4 or C > limit or O > 3 * front.max_channels():
        return None
    if not point_attention._fusable(self.attn, point):
        return None
    return conv, lin, lnc, ln1, qkv


def install(pt_v3_module, max_channels=None):
    """Have Block.forward of the caller's imported models.pt_v3 run its front on the fused kernels.  max_channels caps the
    Blocks' width that takes them, never beyond the library's limit.  Idempotent (a new cap is taken over)."""
    if max_channels is not None and (not isinstance(max_channels, int) or max_channels < 0):
        raise ValueError("max_channels must be None or a non-negative int, got %r" % (max_channels,))
    limit = front.max_channels()  # loads the library: a build without the operator fails here, not inside a forward
    if torch.float32 not in attention.dtypes():
        raise RuntimeError("libgca_hip.so has no float32 attention: the fused Block front needs it")
    point_block.turn(pt_v3_module, front=limit if max_channels is None else min(limit, max_channels))


def uninstall(pt_v3_module):
    """Turn the third off.  Block.forward is put back when point_ffn is off too, if it is still point_block's; where
    another binding was made over it, that one stays and point_block's method hands every call to the one it found."""
    point_block.turn(pt_v3_module, front=None)
