"""The middle of the PTv3 point backbone's Block over libgcm_hip.so (include/gcm.h): between the qkv
projection and the feed-forward tail Block.forward runs qkv[order], the attention, feat[inverse], attn.proj Linear(C, C),
proj_drop, DropPath and the residual add.  install() marks a caller's imported models.pt_v3 so that point_front's rebound
Block.forward runs them as mid.gather_rows, attention.varlen_attention and ONE call of mid.proj_residual, and the two
gathers' gradients without a sort.

  install(pt_v3) / uninstall(pt_v3)     set / remove the marker point_front's method looks for
  middle(block, point, feat, qkv)       the Block's middle from the projected qkv [N, 3C] and the shortcut feat [N, C] on
  accepts(block, point, pt_v3)          whether the marker is set and the Block's middle is what the operators compute
  stats() / reset_stats()               calls that took the fused middle, calls handed back to point_front's own lines

The middle needs a Block-level method that holds qkv and the shortcut at once; that method is point_front's.  install()
therefore installs point_front first when its method is not bound (directly or under point_ffn's), with its default cap;
a binding that exists is left as it is.  uninstall() removes only the marker: point_front stays installed, and its method
runs the lines it ran before.  Both install orders with point_ffn work as they do for point_front.

A Block is accepted when point_front accepts it (the caller has checked that), attn.proj is a Linear(C, C) with bias,
proj_drop is inactive (p == 0 or not training), drop_path is an Identity or DropPath-like (point_ffn's test) and C is at
most mid.max_channels().  Everything else runs point_front's own lines.  The DropPath mask is drawn as point_ffn.fused_tail
draws its own, at the position in the RNG stream where upstream's first drop_path draws: the attention draws nothing.
extra, the duplicate-slot vector, is computed per call that needs a gradient (a forward alone does not read it): two small
launches cost less than a cache-validity rule.
"""
import torch

from . import attention, mid, point_attention, point_ffn

_STATS = {"fused_calls": 0, "original_calls": 0}
_MARK = "_gaussiancity_amd_point_mid_installed"


def stats():
    """Counters of this process: Block middles that ran the fused operators, middles handed back while the marker was set."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _parts(self, point):
    """(attn.proj, DropPath or None) when the Block's middle is what the operators compute, else None."""
    attn = self.attn
    proj, proj_drop = getattr(attn, "proj", None), getattr(attn, "proj_drop", None)
    feat = point.feat
    C = feat.shape[1]
    if not isinstance(proj, torch.nn.Linear) or proj.bias is None or proj.in_features != C or proj.out_features != C:
        return None
    if proj_drop is not None and not isinstance(proj_drop, torch.nn.Identity):
        if not hasattr(proj_drop, "p") or (proj_drop.p != 0 and proj_drop.training):
            return None
    drop = point_ffn._only(self.drop_path)
    if isinstance(drop, torch.nn.Identity):
        drop = None
    elif drop is None or not hasattr(drop, "drop_prob") or not hasattr(drop, "scale_by_keep"):
        return None
    if C % 4 or C > mid.max_channels() or getattr(attn, "channels", None) != C:
        return None
    return proj, drop


def accepts(self, point, pt_v3_module):
    """For point_front's method, after its own checks: None without the marker (nothing is counted), else what _parts
    returns; a Block turned away while the marker is set is counted as handed back."""
    if not getattr(pt_v3_module, _MARK, False):
        return None
    parts = _parts(self, point)
    if parts is None:
        _STATS["original_calls"] += 1
    return parts


# ---- the lines of models/pt_v3.py between the projection and the second shortcut, written against their behaviour: the
# attributes SerializedAttention.forward sets, its one wait for the smallest batch element, the keys it reads, and the order
# of gather, attention, scatter, projection, dropout, DropPath and the residual add ----------------------------------------
def middle(self, point, feat, qkv, parts=None):
    """The Block's middle: point.feat = feat + drop_path(proj(attention(qkv[order])[inverse])).  feat [N, C] is the shortcut
    (the Block's features after its first residual add), qkv [N, 3C] the projection; parts is what accepts() returned.
    Counted as a fused call here, in point_attention and, by the caller, in point_front."""
    if parts is None:
        parts = _parts(self, point)
        if parts is None:
            raise ValueError("this Block's middle is not what the fused operators compute")
    proj, drop = parts
    attn = self.attn
    counts = torch.diff(point.offset, prepend=point.offset.new_zeros(1))
    attn.patch_size = min(counts.min().tolist(), attn.patch_size_max)  # forward_from_qkv's one wait
    H, C = attn.num_heads, attn.channels
    pad, unpad, cu_seqlens = attn.get_padding_and_inverse(point)
    order = point.serialized_order[attn.order_index][pad]
    inverse = unpad[point.serialized_inverse[attn.order_index]]
    need = torch.is_grad_enabled() and any(t.requires_grad for t in (qkv, feat, proj.weight, proj.bias))
    extra = mid.slot_plan(order, inverse) if need else None  # only the gradients read it
    packed = mid.gather_rows(qkv, order, inverse, extra)
    out = attention.varlen_attention(packed.reshape(-1, 3, H, C // H), cu_seqlens, max_seqlen=attn.patch_size,
                                     softmax_scale=attn.scale)
    row_scale = None
    if drop is not None and drop.drop_prob and drop.training:  # DropPath._drop_path's mask, drawn as it draws it
        keep = 1 - drop.drop_prob
        row_scale = feat.new_empty((feat.shape[0], 1)).bernoulli_(keep)
        if keep > 0.0 and drop.scale_by_keep:
            row_scale.div_(keep)
    point.feat = mid.proj_residual(out.reshape(-1, C), inverse, extra, feat, proj.weight, proj.bias, row_scale)
    point_attention._STATS["fused_calls"] += 1
    _STATS["fused_calls"] += 1
    return point


def install(pt_v3_module):
    """Mark the caller's imported models.pt_v3 so that point_front's rebound Block.forward runs the fused middle.
    point_front is installed first (default cap) when its method is not bound; idempotent."""
    from . import point_front  # (point_front imports this module)
    mid.max_channels()  # loads the library: a build without the operators fails here, not inside a forward
    bound = getattr(pt_v3_module, point_front._BOUND, None)
    if bound is None or not (pt_v3_module.Block.forward is bound or getattr(pt_v3_module, point_ffn._ORIGINAL, None) is bound):
        point_front.install(pt_v3_module)
    setattr(pt_v3_module, _MARK, True)


def uninstall(pt_v3_module):
    """Remove the marker; point_front stays as it is."""
    if hasattr(pt_v3_module, _MARK):
        delattr(pt_v3_module, _MARK)
