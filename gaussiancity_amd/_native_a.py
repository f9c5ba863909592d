"""ctypes binding of libgca_hip.so (C ABI in include/gca.h): variable-length packed-QKV attention in binary16.
The library is the product: no Python/CPU fallback -- a missing library or failing call raises RuntimeError."""
import ctypes as C
import os

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libgca_hip.so")
EXPORTED_SYMBOLS = ("gca_abi_version", "gca_last_error", "gca_lse_bytes", "gca_backward_workspace_bytes",
                    "gca_varlen_forward", "gca_varlen_backward")
HEAD_DIMS = (16, 32, 64)  # the instantiations of the kernels
ABI_VERSION = 1
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libgca_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C gaussiancity_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, i64, f32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_float
    L.gca_abi_version.restype = C.c_int
    L.gca_last_error.restype = C.c_char_p
    L.gca_lse_bytes.restype = sz
    L.gca_lse_bytes.argtypes = [i64, i32]
    L.gca_backward_workspace_bytes.restype = sz
    L.gca_backward_workspace_bytes.argtypes = [i64, i32]
    L.gca_varlen_forward.restype = C.c_int
    L.gca_varlen_forward.argtypes = [vp, i64, i64, i64, vp, i64, i64, i32, i32, i64, f32, vp, vp, vp]
    L.gca_varlen_backward.restype = C.c_int
    L.gca_varlen_backward.argtypes = [vp, i64, i64, i64, vp, vp, i64, i64, vp, vp, i64, i64, i32, i32, i64, f32, vp, vp,
                                      sz, vp]
    if L.gca_abi_version() != ABI_VERSION:
        raise RuntimeError("libgca_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed (gca_status %d): %s" % (what, rc, lib().gca_last_error().decode("utf-8", "replace")))
    return rc
