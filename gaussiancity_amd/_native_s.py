"""ctypes binding of libgcs_hip.so (C ABI in include/gcs.h): submanifold sparse convolution and segment_csr.
The library is the product: no Python/CPU fallback -- a missing library or failing call raises RuntimeError."""
import ctypes as C
import os

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libgcs_hip.so")
EXPORTED_SYMBOLS = ("gcs_abi_version", "gcs_last_error", "gcs_subm_rulebook_bytes", "gcs_subm_rulebook_scratch_bytes",
                    "gcs_subm_backward_workspace_bytes", "gcs_subm_rulebook", "gcs_subm_forward", "gcs_subm_backward",
                    "gcs_segment_csr_forward", "gcs_segment_csr_backward")
REDUCE = {"sum": 0, "add": 0, "mean": 1, "min": 2, "max": 3}  # enum gcs_reduce
HOST_INFO_HEADER = 2  # GCS_HOST_INFO_HEADER: invalid rows, duplicate flag, then pairs per tap
ABI_VERSION = 1
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libgcs_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C gaussiancity_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, i64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64
    L.gcs_abi_version.restype = C.c_int
    L.gcs_last_error.restype = C.c_char_p
    L.gcs_subm_rulebook_bytes.restype = sz
    L.gcs_subm_rulebook_bytes.argtypes = [i64, i32]
    L.gcs_subm_rulebook_scratch_bytes.restype = sz
    L.gcs_subm_rulebook_scratch_bytes.argtypes = [i64]
    L.gcs_subm_backward_workspace_bytes.restype = sz
    L.gcs_subm_backward_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    L.gcs_subm_rulebook.restype = C.c_int
    L.gcs_subm_rulebook.argtypes = [vp, i64, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), vp, sz, vp, sz,
                                    C.POINTER(i32), vp]
    L.gcs_subm_forward.restype = C.c_int
    L.gcs_subm_forward.argtypes = [vp, i64, i32, vp, i32, vp, vp, i32, vp, vp]
    L.gcs_subm_backward.restype = C.c_int
    L.gcs_subm_backward.argtypes = [vp, i64, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, sz, vp]
    L.gcs_segment_csr_forward.restype = C.c_int
    L.gcs_segment_csr_forward.argtypes = [vp, i64, i64, vp, i64, i32, vp, vp, vp]
    L.gcs_segment_csr_backward.restype = C.c_int
    L.gcs_segment_csr_backward.argtypes = [vp, i64, i64, vp, i64, i32, vp, vp, vp]
    if L.gcs_abi_version() != ABI_VERSION:
        raise RuntimeError("libgcs_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed (gcs_status %d): %s" % (what, rc, lib().gcs_last_error().decode("utf-8", "replace")))
    return rc


def triple(values):
    """Three int32 values for the shape arguments of gcs_subm_rulebook."""
    return (C.c_int32 * 3)(*[int(v) for v in values])
