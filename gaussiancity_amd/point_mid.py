"""The middle of the PTv3 point backbone's Block over libgcm_hip.so (include/gcm.h): between the qkv
projection and the feed-forward tail Block.forward runs qkv[order], the attention, feat[inverse], attn.proj Linear(C, C),
proj_drop, DropPath and the residual add.  install() turns this third on in point_block's rebound method, which then runs
them as mid.gather_rows, attention.varlen_attention and ONE call of mid.proj_residual, and the two gathers' gradients
without a sort.

  install(pt_v3) / uninstall(pt_v3)     turn the third on / off for a caller's imported models.pt_v3
  middle(block, point, feat, qkv)       the Block's middle from the projected qkv [N, 3C] and the shortcut feat [N, C] on
  accepts(block, point, pt_v3)          whether the third is on and the Block's middle is what the operators compute
  stats() / reset_stats()               calls that took the fused middle, calls handed back to the method's own lines

The middle needs qkv and the shortcut at once, which the method holds only after point_front's fused front.  install()
therefore turns point_front on first, with its default cap, when it is off; a cap that is set is left as it is.
uninstall() turns off the middle alone: point_front stays on, and the method runs the lines it ran before.  The middle
alone binds nothing (point_block.py).

A Block is accepted when point_front accepts it (the caller has checked that), attn.proj is a Linear(C, C) with bias,
proj_drop is inactive (p == 0 or not training), drop_path is an Identity or DropPath-like (point_ffn's test) and C is at
most mid.max_channels().  Everything else runs the method's own lines.  The DropPath mask is the one point_ffn.fused_tail
draws for itself, at the position in the RNG stream where upstream's first drop_path draws: the attention draws nothing.
extra, the duplicate-slot vector, is computed per call that needs a gradient (a forward alone does not read it): two small
launches cost less than a cache-validity rule.
"""
import torch

from . import attention, mid, point_attention, point_block, point_ffn, point_front

_STATS = {"fused_calls": 0, "original_calls": 0}


def stats():
    """Counters of this process: Block middles that ran the fused operators, middles handed back while the third was on."""
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
    drop = point_ffn.drop_path_of(self)
    if drop is False or C % 4 or C > mid.max_channels() or getattr(attn, "channels", None) != C:
        return None
    return proj, drop


def accepts(self, point, pt_v3_module):
    """For the rebound method, after point_front's checks: None while the third is off (nothing is counted), else what
    _parts returns; a Block turned away while it is on is counted as handed back."""
    st = point_block.state(pt_v3_module)
    if st is None or not st.mid:
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
    order, inverse, cu_seqlens = point_attention.patches(attn, point)  # forward_from_qkv's one wait
    H, C = attn.num_heads, attn.channels
    need = torch.is_grad_enabled() and any(t.requires_grad for t in (qkv, feat, proj.weight, proj.bias))
    extra = mid.slot_plan(order, inverse) if need else None  # only the gradients read it
    packed = mid.gather_rows(qkv, order, inverse, extra)
    out = attention.varlen_attention(packed.reshape(-1, 3, H, C // H), cu_seqlens, max_seqlen=attn.patch_size,
                                     softmax_scale=attn.scale)
    row_scale = point_ffn.row_scale(drop, feat)
    point.feat = mid.proj_residual(out.reshape(-1, C), inverse, extra, feat, proj.weight, proj.bias, row_scale)
    point_attention._STATS["fused_calls"] += 1
    _STATS["fused_calls"] += 1
    return point


def install(pt_v3_module):
    """Have Block.forward of the caller's imported models.pt_v3 run the fused middle after point_front's front, which is
    turned on first (default cap) when it is off; idempotent."""
    mid.max_channels()  # loads the library: a build without the operators fails here, not inside a forward
    st = point_block.state(pt_v3_module)
    if st is None or st.front is None:
        point_front.install(pt_v3_module)
    point_block.turn(pt_v3_module, mid=True)


def uninstall(pt_v3_module):
    """Turn off the middle alone; point_front stays as it is."""
    point_block.turn(pt_v3_module, mid=False)
