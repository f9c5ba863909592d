"""ctypes binding of libgce_hip.so (C ABI in include/gce.h): multi-resolution hash-grid encoder.  The declarations;
gaussiancity_amd/_loader.py loads it.
The library is the product: no Python/CPU fallback -- a missing library or failing call raises RuntimeError."""
import ctypes as C

from . import _loader

DTYPE_F32, DTYPE_F16, DTYPE_F64 = 0, 1, 2  # enum gce_dtype
STAGE_NAMES = ("forward", "backward_embeddings", "backward_inputs")
ABI_VERSION = 3

_vp, _u32, _f32, _int = C.c_void_p, C.c_uint32, C.c_float, C.c_int
_SIGNATURES = {  # every function include/gce.h declares: name -> (restype, argtypes)
    "gce_abi_version": (_int, []),
    "gce_last_error": (C.c_char_p, []),
    "gce_level_scales": (_int, [_u32, _f32, _u32, C.POINTER(_f32)]),
    "gce_forward": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _u32, _int, _vp]),
    "gce_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _vp, _u32, _int, _vp]),
    "gce_set_option": (_int, [C.c_char_p, _int]),
    "gce_get_stage_ms": (_int, [C.POINTER(_f32), _int]),
    "gce_forward_t": (_int, [_int, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _u32, _int, _vp]),
    "gce_backward_t": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _vp, _u32, _int,
                              _vp]),
    "gce_backward_det_workspace_bytes": (C.c_size_t, [_u32, _u32, _u32, _u32]),
    "gce_backward_det": (_int, [_int, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _f32, _u32, _int, _vp, _vp, _u32, _int,
                                _vp, C.c_size_t, _vp]),
}

_L = _loader.Library("gce", "libgce_hip.so", ABI_VERSION, _SIGNATURES, STAGE_NAMES)
LIB_PATH, EXPORTED_SYMBOLS = _L.path, _L.exported_symbols
lib, check, set_option, stage_ms = _L.lib, _L.check, _L.set_option, _L.stage_ms
