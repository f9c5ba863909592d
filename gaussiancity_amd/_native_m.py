"""ctypes binding of libgcm_hip.so (C ABI in include/gcm.h): the grouped modulated linear layer of the generator's
attribute head, its backward, the group vector from masks and the head's output transform, and the feed-forward third
of a PTv3 Block (gcm_ffn_*: LayerNorm, MLP and residual in one launch, its backward) and the front of the same Block
(gcm_front_*: the convolution's Linear and LayerNorm, the residual, norm1 and the qkv projection in one launch, its backward)
and the middle of the same Block (gcm_mid_*: the patch gather and its gradient, the scatter back, the output projection,
DropPath and the residual in one launch, its backward) and the seams between the backbone's stages (gcm_seam_*: Linear,
BatchNorm1d and GELU as one operator in eval and training mode, its backward) and the attribute head at inference in one
launch per output key (gcm_head_chain) and the head's output layers in a training step (gcm_head_train_*: up to four keys,
the transform and the [N, 14] record in one launch, a backward of two), all float32.  The declarations; gaussiancity_amd/_loader.py loads it.
The library is the product: no Python/CPU fallback -- a missing library or failing call raises RuntimeError."""
import ctypes as C

from . import _loader

ABI_VERSION = 1
KINDS = {"xyz": 0, "rgb": 1, "scale": 2, "opacity": 3}  # enum gcm_kind, by the head's name of the attribute

_vp, _sz, _i32, _i64, _f32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_float


class HeadKey(C.Structure):
    """gcm_head_key: one key of gcm_head_train_forward / gcm_head_train_backward (strides in elements)."""
    _fields_ = [("kind", _i32), ("factor", _f32), ("h", _vp), ("h_stride", _i64), ("w", _vp), ("b", _vp), ("out", _vp),
                ("out_stride", _i64), ("dout", _vp), ("dout_stride", _i64), ("dh", _vp), ("dh_stride", _i64), ("dw", _vp),
                ("db", _vp)]


_keys = C.POINTER(HeadKey)
_SIGNATURES = {  # every function include/gcm.h declares: name -> (restype, argtypes)
    "gcm_abi_version": (C.c_int, []),
    "gcm_last_error": (C.c_char_p, []),
    "gcm_groups_from_masks": (C.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "gcm_modlinear_forward": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _vp, _i64,
                                        _vp]),
    "gcm_modlinear_backward_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "gcm_modlinear_backward": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _f32,
                                         _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcm_head_out": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, C.c_int, _f32, _vp, _vp]),
    "gcm_ffn_max_channels": (C.c_int, []),
    "gcm_ffn_forward": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp,
                                  _vp, _vp]),
    "gcm_ffn_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "gcm_ffn_backward": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcm_ffn_split_max_channels": (C.c_int, []),
    "gcm_ffn_split_plan": (C.c_int, [_i64, _i32, _i32, C.POINTER(_i64)]),
    "gcm_ffn_split_workspace_bytes": (C.c_int, [_i64, _i32, _i32, C.POINTER(_sz), C.POINTER(_sz)]),
    "gcm_ffn_split_forward": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp,
                                        _vp, _vp, _vp, _sz, _vp]),
    "gcm_ffn_split_backward": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp,
                                         _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcm_front_max_channels": (C.c_int, []),
    "gcm_front_forward": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _i64, _i32, _i32,
                                    _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gcm_front_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "gcm_front_backward": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp,
                                     _vp, _i64, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _sz, _vp]),
    "gcm_mid_max_channels": (C.c_int, []),
    "gcm_mid_slot_plan": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "gcm_mid_gather_forward": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp]),
    "gcm_mid_gather_backward": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp]),
    "gcm_mid_forward": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "gcm_mid_backward_workspace_bytes": (_sz, [_i64, _i32]),
    "gcm_mid_backward": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcm_seam_max_channels": (C.c_int, []),
    "gcm_seam_forward_eval": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _f32, _vp, _vp, C.c_int, _i64, _i32, _i32, _vp, _i64,
                                        _vp, _vp, _vp]),
    "gcm_seam_forward_workspace_bytes": (_sz, [_i64, _i32]),
    "gcm_seam_forward_train": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _f32, _vp, _vp, C.c_int, _i64, _i32, _i32, _vp, _vp, _i64,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcm_seam_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "gcm_seam_backward": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, C.c_int, C.c_int, _i64, _i32, _i32,
                                    _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcm_head_chain_max_hidden": (C.c_int, []),
    "gcm_head_chain_max_in": (C.c_int, []),
    "gcm_head_chain": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                 _i32, _i32, _i32, _i32, _i32, C.c_int, _f32, _f32, _vp, _vp]),
    "gcm_head_train_max_in": (C.c_int, []),
    "gcm_head_train_pre_floats": (C.c_int, []),
    "gcm_head_train_plan": (C.c_int, [_i64, _i32, C.POINTER(_i64)]),
    "gcm_head_train_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "gcm_head_train_forward": (C.c_int, [_keys, _i32, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "gcm_head_train_backward": (C.c_int, [_keys, _i32, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _sz, _vp]),
}

_L = _loader.Library("gcm", "libgcm_hip.so", ABI_VERSION, _SIGNATURES)
LIB_PATH, EXPORTED_SYMBOLS = _L.path, _L.exported_symbols
lib, check = _L.lib, _L.check
