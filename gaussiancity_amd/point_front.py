"""The front of the PTv3 point backbone's Block over libgcm_hip.so (include/gcm.h): between its sparse
convolution and its attention Block.forward runs cpe[1] Linear(C, C), cpe[2] LayerNorm(C), the residual add, norm1
LayerNorm(C) and attn.qkv Linear(C, 3C) -- five launches forward and about fourteen backward; install() rebinds the method so
that they are one call of front.conv_tail_norm_qkv.

  install(pt_v3, max_channels=None) / uninstall(pt_v3)     rebind Block.forward of a caller's imported models.pt_v3
  stats() / reset_stats()               calls that took the fused front, calls that went to the method bound at install

The rebound method runs the convolution through its module (the sparse drop-ins keep composing), the attention from the
projection on through point_attention.forward_from_qkv (point_attention.install need not have been called), and the tail
through point_ffn's fused tail when point_ffn is installed on the same module and accepts the Block, else through norm2,
mlp and drop_path themselves.  The DropPath masks are drawn in upstream's order; the front draws nothing.  max_channels
caps the width that goes to the fused front (narrow Blocks have the rows that fill the device), the
default is the library's limit.  post-norm Blocks, another cpe, other norm layers, an attention that point_attention does
not run, CPU tensors, other dtypes, an active autocast and wider Blocks go to the method that was bound at install, untouched.

point_ffn and point_front compose in either install order, and after both uninstalls, in either order, Block.forward is the
module's own method.
"""
import torch

from . import attention, front, point_attention, point_ffn, point_mid

_STATS = {"fused_calls": 0, "original_calls": 0}
_ORIGINAL = "_gaussiancity_amd_point_front_original"
_BOUND = "_gaussiancity_amd_point_front_bound"
_CAP = "_gaussiancity_amd_point_front_max_channels"


def stats():
    """Counters of this process: forwards whose front ran the fused kernels, forwards handed to the method bound at install."""
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
    cap = getattr(pt_v3_module, _CAP, None)
    limit = front.max_channels() if cap is None else min(front.max_channels(), cap)
    if C % 4 or O % 4 or C > limit or O > 3 * front.max_channels():
        return None
    if not point_attention._fusable(self.attn, point):
        return None
    return conv, lin, lnc, ln1, qkv


# ---- the method of models/pt_v3.py, written against its behaviour: the order of its modules, of its residual adds and of
# the DropPath draws, and the attributes it sets on the point ---------------------------------------------------------------
def _forward(original, pt_v3_module):
    def accepts(self, point):
        return getattr(pt_v3_module, _BOUND, None) is forward and _parts(self, point, pt_v3_module) is not None

    def forward(self, point):
        """Block.forward (pre_norm) with everything between the sparse convolution and the attention over
        front.conv_tail_norm_qkv.  From the convolution to the end of the method point.sparse_conv_feat holds the
        convolution's output where upstream holds cpe's; nothing reads it there, and the method's last line sets it."""
        if getattr(pt_v3_module, _BOUND, None) is not forward:  # uninstalled while another binding still holds this method
            return original(self, point)
        parts = _parts(self, point, pt_v3_module)
        if parts is None:
            _STATS["original_calls"] += 1
            return original(self, point)
        conv, lin, lnc, ln1, qkv = parts
        x = point.feat
        point.sparse_conv_feat = conv(point.sparse_conv_feat)  # as PointSequential runs a spconv module
        feat, proj = front.conv_tail_norm_qkv(x, point.sparse_conv_feat.features, lin.weight, lin.bias, lnc.weight, lnc.bias,
                                              lnc.eps, ln1.weight, ln1.bias, ln1.eps, qkv.weight, qkv.bias)
        point.feat = feat
        middle = point_mid.accepts(self, point, pt_v3_module)  # None without point_mid's marker
        if middle is not None:
            point = point_mid.middle(self, point, feat, proj, middle)
        else:
            point = self.drop_path(point_attention.forward_from_qkv(self.attn, point, proj))
            point.feat = feat + point.feat
        _STATS["fused_calls"] += 1

        tail = point_ffn._parts(self, point, pt_v3_module) if getattr(pt_v3_module, point_ffn._ORIGINAL, None) is not None else None
        if tail is not None:
            return point_ffn.fused_tail(point, tail, point_ffn.takes_split(pt_v3_module, point.feat.shape[1]))
        shortcut = point.feat
        point = self.norm2(point)
        point = self.drop_path(self.mlp(point))
        point.feat = shortcut + point.feat
        point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
        return point
    forward.block_front_accepts = accepts  # point_ffn, bound over this method, hands it the Blocks it accepts
    return forward


def install(pt_v3_module, max_channels=None):
    """Rebind Block.forward of the caller's imported models.pt_v3 so that its front runs the fused kernels.  max_channels
    caps the Blocks' width that takes them.  Idempotent while its method is the one bound, directly or under point_ffn's
    (a new cap is taken over); when another module's uninstall has put a different method on Block.forward since, it binds
    again."""
    if max_channels is not None and (not isinstance(max_channels, int) or max_channels < 0):
        raise ValueError("max_channels must be None or a non-negative int, got %r" % (max_channels,))
    bound = getattr(pt_v3_module, _BOUND, None)
    if bound is not None and (pt_v3_module.Block.forward is bound or getattr(pt_v3_module, point_ffn._ORIGINAL, None) is bound):
        setattr(pt_v3_module, _CAP, max_channels)
        return  # still bound, directly or under point_ffn's method, which was installed over it
    front.max_channels()  # loads the library: a build without the operator fails here, not inside a forward
    if torch.float32 not in attention.dtypes():
        raise RuntimeError("libgca_hip.so has no float32 attention: the fused Block front needs it")
    original = pt_v3_module.Block.forward
    bound = _forward(original, pt_v3_module)
    for name, value in ((_ORIGINAL, original), (_BOUND, bound), (_CAP, max_channels)):
        setattr(pt_v3_module, name, value)
    pt_v3_module.Block.forward = bound


def uninstall(pt_v3_module):
    """Put back the method install() found, if Block.forward is still install()'s; otherwise (another binding was made over
    it, or removed it) only the marker goes: the method then hands every call to the one it found."""
    bound = getattr(pt_v3_module, _BOUND, None)
    if bound is None:
        return
    original = getattr(pt_v3_module, _ORIGINAL)
    if pt_v3_module.Block.forward is bound:
        pt_v3_module.Block.forward = original
    elif getattr(pt_v3_module, point_ffn._ORIGINAL, None) is bound:  # point_ffn, installed later, would restore this method
        setattr(pt_v3_module, point_ffn._ORIGINAL, original)
    for name in (_ORIGINAL, _BOUND, _CAP):
        delattr(pt_v3_module, name)
