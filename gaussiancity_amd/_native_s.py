"""ctypes binding of libgcs_hip.so (C ABI in include/gcs.h): submanifold sparse convolution and segment_csr.  The
declarations; gaussiancity_amd/_loader.py loads it.
The library is the product: no Python/CPU fallback -- a missing library or failing call raises RuntimeError."""
import ctypes as C

from . import _loader

REDUCE = {"sum": 0, "add": 0, "mean": 1, "min": 2, "max": 3}  # enum gcs_reduce
TILE_32X32, TILE_64X64, TILE_128X32 = 0, 1, 2  # enum gcs_tile
HOST_INFO_HEADER = 2  # GCS_HOST_INFO_HEADER: invalid rows, duplicate flag, then pairs per tap
ENGINE_VALU, ENGINE_MFMA = 0, 1  # enum gcs_engine
ENGINES = {"valu": ENGINE_VALU, "mfma": ENGINE_MFMA}
PRODUCT_FORWARD, PRODUCT_DX, PRODUCT_DW = 1, 2, 4  # GCS_PRODUCT_*: the bits of gcs_engine_products
DTYPE_F32, DTYPE_F16 = 0, 1  # enum gcs_dtype
DTYPES = {"float32": DTYPE_F32, "float16": DTYPE_F16}  # the `_t` entry points; gcs_dtypes() says which the library runs
ORDERS = {"cord": 0, "z": 1, "z-trans": 2, "hilbert": 3, "hilbert-trans": 4}  # enum gcs_order; gcs_index_orders() has the bits
ABI_VERSION = 4

_vp, _sz, _i32, _i64, _int = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_int
_pi32 = C.POINTER(_i32)
_psz = C.POINTER(_sz)
_SIGNATURES = {  # every function include/gcs.h declares: name -> (restype, argtypes)
    "gcs_abi_version": (_int, []),
    "gcs_last_error": (C.c_char_p, []),
    "gcs_subm_rulebook_bytes": (_sz, [_i64, _i32]),
    "gcs_subm_rulebook_scratch_bytes": (_sz, [_i64]),
    "gcs_subm_backward_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "gcs_subm_plan": (_int, [_i64, _i32, _i32, _i32, _pi32]),
    "gcs_subm_rulebook": (_int, [_vp, _i64, _i32, _pi32, _pi32, _pi32, _vp, _sz, _vp, _sz, _pi32, _vp]),
    "gcs_subm_forward": (_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "gcs_subm_backward": (_int, [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcs_engine_products": (_int, [_i32]),
    "gcs_subm_engine_plan": (_int, [_i32, _i64, _i32, _i32, _i32, _pi32]),
    "gcs_subm_engine_workspace_bytes": (_int, [_i32, _i64, _i32, _i32, _i32, _i32, _psz, _psz]),
    "gcs_subm_forward_engine": (_int, [_i32, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gcs_subm_backward_engine": (_int, [_i32, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz,
                                        _vp]),
    "gcs_segment_csr_forward": (_int, [_vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    "gcs_segment_csr_backward": (_int, [_vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    "gcs_dtypes": (_int, []),
    "gcs_subm_workspace_bytes_t": (_int, [_i32, _i64, _i32, _i32, _i32, _i32, _psz, _psz]),
    "gcs_subm_forward_t": (_int, [_i32, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gcs_subm_backward_t": (_int, [_i32, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcs_segment_csr_forward_t": (_int, [_i32, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    "gcs_segment_csr_backward_t": (_int, [_i32, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp]),
    "gcs_index_orders": (_int, []),
    "gcs_serialize_workspace_bytes": (_sz, [_i64, _i32]),
    "gcs_serialize": (_int, [_vp, _vp, _i64, _i32, _i32, C.c_float, C.c_float, _pi32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcs_patch_plan_count": (_int, [_vp, _i32, _i64, _vp, _vp]),
    "gcs_patch_plan_emit": (_int, [_vp, _i32, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "gcs_pool_reduces": (_int, []),
    "gcs_pool_plan_workspace_bytes": (_sz, [_i64, _i32]),
    "gcs_pool_plan_count": (_int, [_vp, _i32, _i64, _i32, _vp, _sz, _vp, _vp]),
    "gcs_pool_plan_emit": (_int, [_vp, _i32, _i64, _i32, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gcs_segment_gather_forward_t": (_int, [_i32, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "gcs_segment_gather_backward_t": (_int, [_i32, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp]),
    "gcs_segment_expand_add_t": (_int, [_i32, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
}

_L = _loader.Library("gcs", "libgcs_hip.so", ABI_VERSION, _SIGNATURES)
LIB_PATH, EXPORTED_SYMBOLS = _L.path, _L.exported_symbols
lib, check = _L.lib, _L.check


def triple(values):
    """Three int32 values for the shape arguments of gcs_subm_rulebook."""
    return (C.c_int32 * 3)(*[int(v) for v in values])


def subm_plan(n, cin, cout, kvol):
    """(forward tile, dX tile, dW tile, dW slices, dB slices) of gcs_subm_plan: what the library launches for the shape."""
    out = (C.c_int32 * 5)()
    check(lib().gcs_subm_plan(n, cin, cout, kvol, out), "gcs_subm_plan")
    return tuple(out)


def engine_products(engine):
    """gcs_engine_products: the PRODUCT_* bits of what `engine` runs on the matrix cores (0 for VALU, 7 for MFMA)."""
    return check(lib().gcs_engine_products(engine), "gcs_engine_products")


def subm_engine_plan(engine, n, cin, cout, kvol):
    """gcs_subm_engine_plan: subm_plan's five values, then the tap slices of the forward and of dX (1, 1 for VALU)."""
    out = (C.c_int32 * 7)()
    check(lib().gcs_subm_engine_plan(engine, n, cin, cout, kvol, out), "gcs_subm_engine_plan")
    return tuple(out)


def subm_engine_workspace_bytes(engine, n, cin, cout, kvol, dups):
    """(forward bytes, backward bytes) of gcs_subm_engine_workspace_bytes; the forward's are 0 with one tap slice."""
    f, b = _sz(0), _sz(0)
    check(lib().gcs_subm_engine_workspace_bytes(engine, n, cin, cout, kvol, dups, C.byref(f), C.byref(b)),
          "gcs_subm_engine_workspace_bytes")
    return int(f.value), int(b.value)


def dtypes():
    """gcs_dtypes: the names out of DTYPES that the library runs, in enum order."""
    bits = lib().gcs_dtypes()
    return tuple(name for name, code in DTYPES.items() if bits >> code & 1)


def subm_workspace_bytes_t(dtype, n, cin, cout, kvol, dups):
    """(forward bytes, backward bytes) of gcs_subm_workspace_bytes_t for the DTYPE_* code `dtype`."""
    f, b = _sz(0), _sz(0)
    check(lib().gcs_subm_workspace_bytes_t(dtype, n, cin, cout, kvol, dups, C.byref(f), C.byref(b)),
          "gcs_subm_workspace_bytes_t")
    return int(f.value), int(b.value)
