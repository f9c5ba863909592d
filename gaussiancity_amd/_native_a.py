"""ctypes binding of libgca_hip.so (C ABI in include/gca.h): variable-length packed-QKV attention in binary16 and
float32.  The declarations; gaussiancity_amd/_loader.py loads it.
The library is the product: no Python/CPU fallback -- a missing library or failing call raises RuntimeError."""
import ctypes as C

from . import _loader

HEAD_DIMS = (16, 32, 64)  # the instantiations of the kernels
ABI_VERSION = 1
DTYPES = {"float16": 0, "float32": 1}  # enum gca_dtype, by torch's name of the type

_vp, _sz, _i32, _i64, _f32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_float
_SIGNATURES = {  # every function include/gca.h declares: name -> (restype, argtypes)
    "gca_abi_version": (C.c_int, []),
    "gca_last_error": (C.c_char_p, []),
    "gca_lse_bytes": (_sz, [_i64, _i32]),
    "gca_backward_workspace_bytes": (_sz, [_i64, _i32]),
    "gca_varlen_forward": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i64, _f32, _vp, _vp, _vp]),
    "gca_varlen_backward": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i64,
                                      _f32, _vp, _vp, _sz, _vp]),
    "gca_dtypes": (C.c_int, []),
    "gca_varlen_forward_t": (C.c_int, [C.c_int, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i64, _f32, _vp, _vp, _vp]),
    "gca_varlen_backward_t": (C.c_int, [C.c_int, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32,
                                        _i64, _f32, _vp, _vp, _sz, _vp]),
}

_L = _loader.Library("gca", "libgca_hip.so", ABI_VERSION, _SIGNATURES)
LIB_PATH, EXPORTED_SYMBOLS = _L.path, _L.exported_symbols
lib, check = _L.lib, _L.check
