"""The one owner of Block.forward of the PTv3 point backbone: point_front, point_mid and point_ffn each
fuse a third of the method, and which thirds are on is one record per models.pt_v3 namespace.

  state(pt_v3)              the record, or None when no third is on: original, bound, front, mid, ffn
  turn(pt_v3, front=..., mid=..., ffn=...)      what the three installs and uninstalls call: set fields, bind or put back

front is None or the widest Block the fused front takes, mid is False or True, ffn is None or (max_channels, split).
Block.forward is bound once, when front or ffn first turns on, over whatever is there; the function stays the same object
while either is on and is put back when both are off, if Block.forward is still that function.  Where someone else has
bound over it, the foreign method stays; our function, if that method still reaches it, finds no record of itself and
hands every call to the method it found.  mid alone binds nothing.  The record leaves the namespace with the last third.
"""
_STATE = "_gaussiancity_amd_point_block"


class _State:
    __slots__ = ("original", "bound", "front", "mid", "ffn")

    def __init__(self):
        self.original = self.bound = self.front = self.ffn = None
        self.mid = False


def state(pt_v3_module):
    """The record of the thirds that are on for this models.pt_v3, or None."""
    return getattr(pt_v3_module, _STATE, None)


def turn(pt_v3_module, **fields):
    """Set the given fields of the record and make Block.forward follow them."""
    st = state(pt_v3_module) or _State()
    for name, value in fields.items():
        setattr(st, name, value)
    wanted = st.front is not None or st.ffn is not None
    if wanted and st.bound is None:
        st.original = pt_v3_module.Block.forward
        pt_v3_module.Block.forward = st.bound = _forward(st.original, pt_v3_module)
    elif not wanted and st.bound is not None:
        if pt_v3_module.Block.forward is st.bound:
            pt_v3_module.Block.forward = st.original
        st.original = st.bound = None
    if wanted or st.mid:
        setattr(pt_v3_module, _STATE, st)
    elif state(pt_v3_module) is not None:
        delattr(pt_v3_module, _STATE)


# ---- the method of models/pt_v3.py, written against its behaviour: the order of its modules, of its residual adds and of
# the DropPath draws, and the attributes it sets on the point ---------------------------------------------------------------
def _forward(original, pt_v3_module):
    from . import front, point_attention, point_ffn, point_front, point_mid  # (the three import this module)

    def forward(self, point):
        """Block.forward (pre_norm) with the thirds that are on over their fused operators.  With the front on, from the
        convolution to the end of the method point.sparse_conv_feat holds the convolution's output where upstream holds
        cpe's; nothing reads it there, and the method's last line sets it."""
        st = state(pt_v3_module)
        if st is None or st.bound is not forward:  # put away while another binding still holds this method
            return original(self, point)
        fp = None
        if st.front is not None:
            fp = point_front._parts(self, point, pt_v3_module)
            if fp is None:
                point_front._STATS["original_calls"] += 1
        if fp is None:
            tp = point_ffn._parts(self, point, pt_v3_module) if st.ffn is not None else None
            if tp is None:
                if st.ffn is not None:
                    point_ffn._STATS["original_calls"] += 1
                return original(self, point)
            shortcut = point.feat
            point = self.cpe(point)
            point.feat = shortcut + point.feat
            shortcut = point.feat
            point = self.norm1(point)
            point = self.drop_path(self.attn(point))
            point.feat = shortcut + point.feat
            return point_ffn.fused_tail(point, tp, point_ffn.takes_split(pt_v3_module, point.feat.shape[1]))
        conv, lin, lnc, ln1, qkv = fp
        x = point.feat
        point.sparse_conv_feat = conv(point.sparse_conv_feat)  # as PointSequential runs a spconv module
        feat, proj = front.conv_tail_norm_qkv(x, point.sparse_conv_feat.features, lin.weight, lin.bias, lnc.weight, lnc.bias,
                                              lnc.eps, ln1.weight, ln1.bias, ln1.eps, qkv.weight, qkv.bias)
        point.feat = feat
        middle = point_mid.accepts(self, point, pt_v3_module)  # None while mid is off
        if middle is not None:
            point = point_mid.middle(self, point, feat, proj, middle)
        else:
            point = self.drop_path(point_attention.forward_from_qkv(self.attn, point, proj))
            point.feat = feat + point.feat
        point_front._STATS["fused_calls"] += 1

        tp = point_ffn._parts(self, point, pt_v3_module) if st.ffn is not None else None
        if tp is not None:
            return point_ffn.fused_tail(point, tp, point_ffn.takes_split(pt_v3_module, point.feat.shape[1]))
        shortcut = point.feat
        point = self.norm2(point)
        point = self.drop_path(self.mlp(point))
        point.feat = shortcut + point.feat
        point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
        return point
    return forward
