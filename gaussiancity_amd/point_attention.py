"""The attention of the PTv3 point backbone's DEFAULT branch over libgca_hip.so (include/gca.h):
SerializedAttention.forward with enable_flash=False computes (q * scale) @ k^T, softmax and @ v on [patches, H, K, K]
tensors; install() rebinds the method so that this branch runs the fused kernels of attention.varlen_attention in the
features' own dtype -- float32 features in fp32 throughout, float16 features (autocast) on the binary16 kernels.

  install(pt_v3) / uninstall(pt_v3)     rebind SerializedAttention.forward of a caller's imported models.pt_v3
  stats() / reset_stats()               calls that took the fused path, calls that went to the module's own method
  forward_from_qkv(attn, point, qkv)    the rebound method from the qkv projection on, for a caller that has the
                                        projection already (point_front computes it in the Block front's one launch)
  patches(attn, point)                  the method's patch size, row orders and patch bounds (point_mid's middle shares them)

Independent of point_index.install: the rebound method calls self.get_padding_and_inverse, whoever provides it.  Relative
position encoding, active attention dropout, the flash branch, CPU tensors and other dtypes go to the module's own method,
untouched.
"""
import torch

from . import attention

_STATS = {"fused_calls": 0, "original_calls": 0}
_ORIGINAL = "_gaussiancity_amd_point_attention_original"


def stats():
    """Counters of this process: forwards that ran the fused kernels, forwards handed to the module's own method."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _fusable(self, point):
    """Everything but the dtype, which only the projection's output tells."""
    if self.enable_flash or self.enable_rpe:
        return False
    if self.attn_drop.p != 0 and self.training:
        return False
    if not point.feat.is_cuda:
        return False
    return self.channels // self.num_heads in attention.SUPPORTED_HEAD_DIMS


# ---- the method of models/pt_v3.py, written against its behaviour: the attributes it sets, its one wait for the smallest
# batch element, the keys it reads, and the order of gather, attention, scatter, projection and dropout ----------------
def patches(self, point):
    """(order, inverse, cu_seqlens) of the method's patches: the rows in padded serialized order, each point's row there,
    the patch bounds.  Sets self.patch_size as the method does, which is its one wait."""
    counts = torch.diff(point.offset, prepend=point.offset.new_zeros(1))
    self.patch_size = min(counts.min().tolist(), self.patch_size_max)
    pad, unpad, cu_seqlens = self.get_padding_and_inverse(point)
    order = point.serialized_order[self.order_index][pad]
    inverse = unpad[point.serialized_inverse[self.order_index]]
    return order, inverse, cu_seqlens


def forward_from_qkv(self, point, qkv):
    """SerializedAttention.forward's non-flash branch from the projected qkv [N, 3C] on, over attention.varlen_attention:
    the caller has checked _fusable(self, point) and that qkv's dtype is one of attention.dtypes().  Counted as a fused call."""
    order, inverse, cu_seqlens = patches(self, point)
    H, C = self.num_heads, self.channels
    feat = attention.varlen_attention(qkv[order].reshape(-1, 3, H, C // H), cu_seqlens, max_seqlen=self.patch_size,
                                      softmax_scale=self.scale)
    feat = feat.reshape(-1, C)[inverse]
    point.feat = self.proj_drop(self.proj(feat))
    _STATS["fused_calls"] += 1
    return point


def _forward(original):
    def forward(self, point):
        """SerializedAttention.forward's non-flash branch over attention.varlen_attention."""
        qkv = self.qkv(point.feat) if _fusable(self, point) else None
        if qkv is None or qkv.dtype not in attention.dtypes():
            _STATS["original_calls"] += 1
            return original(self, point)
        return forward_from_qkv(self, point, qkv)
    return forward


def install(pt_v3_module):
    """Rebind SerializedAttention.forward of the caller's imported models.pt_v3 to the fused kernels.  Idempotent;
    uninstall() puts the module's own method back."""
    if getattr(pt_v3_module, _ORIGINAL, None) is not None:
        return
    attention.dtypes()  # loads the library: a build without the typed entry points fails here, not inside a forward
    original = pt_v3_module.SerializedAttention.forward
    setattr(pt_v3_module, _ORIGINAL, original)
    pt_v3_module.SerializedAttention.forward = _forward(original)


def uninstall(pt_v3_module):
    original = getattr(pt_v3_module, _ORIGINAL, None)
    if original is None:
        return
    pt_v3_module.SerializedAttention.forward = original
    delattr(pt_v3_module, _ORIGINAL)
