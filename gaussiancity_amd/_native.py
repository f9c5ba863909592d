"""ctypes binding of libgcr_hip.so (C ABI in include/gcr.h): the declarations; gaussiancity_amd/_loader.py loads it.

The library is the product: there is NO Python/CPU fallback.  If it is missing or a call
fails, a RuntimeError is raised (the reference surfaces native failures the same way:
C++ exceptions -> RuntimeError, dgr/rasterize_points.cu:46-48, cr/auxiliary.h:158-167).
"""
import ctypes as C
import subprocess

from . import _loader

GRAD_REC_FLOATS = 16  # gcr_grad_record_floats() by default (32 under option "deterministic_backward": ext asks per call)

STAGE_NAMES = ("preprocess", "scan", "emit", "sort", "ranges", "blend_fwd", "blend_bwd",
               "preprocess_bwd")


class Options(C.Structure):
    """gcr_options: per-call overrides of the gcr_set_option() defaults (-1 = the default)."""
    _fields_ = [(n, C.c_int32) for n in (
        "lazy_sort", "sort_in_blend", "bwd_piece", "deterministic_backward", "split_preprocess",
        "force_radix", "force_global_cursor", "bwd_wave_units")]

    def __init__(self, **kw):
        super().__init__(*([-1] * 8))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown rasterizer option %r" % k)
            setattr(self, k, int(v))


class Camera(C.Structure):
    """gcr_camera == GaussianRasterizationSettings (dgr/__init__.py:203-215)."""
    _fields_ = [
        ("img_h", C.c_int32), ("img_w", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float),
        ("scale_modifier", C.c_float), ("sh_degree", C.c_int32),
        ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("bg", C.c_void_p), ("view_matrix", C.c_void_p),
        ("proj_matrix", C.c_void_p), ("campos", C.c_void_p),
        ("host_camera", C.c_int32),  # bg/view/proj/campos are host pointers (copied into the kernel arguments)
        ("flip_x", C.c_int32), ("flip_y", C.c_int32),  # mirrored image store / gradient load
        ("win_x", C.c_int32), ("win_y", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32),  # output window
        ("backward", C.c_int32),  # 1: a backward call will follow (the forward blend leaves its per-piece state)
        ("options", C.POINTER(Options)),  # per-call options or NULL
        ("out_u8", C.c_int32),  # out_color is a uint8 [H,W,3] video frame (inference frames)
    ]


class Gaussians(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("M", C.c_int32),
        ("means3D", C.c_void_p), ("opacities", C.c_void_p), ("shs", C.c_void_p),
        ("colors_precomp", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p),
        ("cov3D_precomp", C.c_void_p),
        ("stride_means3D", C.c_int32), ("stride_opacities", C.c_int32), ("stride_colors", C.c_int32),
        ("stride_scales", C.c_int32), ("stride_rotations", C.c_int32),
        ("cull_cache", C.c_void_p),  # ABI v8: gcr_cull_cache_bytes(P) bytes of gcr_build_cull_cache, or NULL
    ]


class Grads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D",
        "dL_dsh", "dL_dscales", "dL_drotations")] + [
        ("stride_means3D", C.c_int32), ("stride_opacity", C.c_int32), ("stride_colors", C.c_int32),
        ("stride_scales", C.c_int32), ("stride_rotations", C.c_int32),
        ("packed", C.c_void_p), ("packed_floats", C.c_int64)]


class Layout(C.Structure):
    _fields_ = [
        ("geom_rec", C.c_size_t), ("geom_cov3D", C.c_size_t), ("geom_clamped", C.c_size_t),
        ("geom_tiles_touched", C.c_size_t), ("geom_block_sums", C.c_size_t),
        ("geom_vis_list", C.c_size_t), ("geom_vis_count", C.c_size_t),
        ("geom_num_rendered", C.c_size_t), ("geom_block_tiles", C.c_size_t), ("geom_total", C.c_size_t),
        ("img_final_T", C.c_size_t), ("img_n_contrib", C.c_size_t), ("img_ranges", C.c_size_t),
        ("img_tile_cursor", C.c_size_t), ("img_tile_table", C.c_size_t), ("img_tile_lazy", C.c_size_t),
        ("img_total", C.c_size_t),
        ("bin_keys", C.c_size_t * 2), ("bin_vals", C.c_size_t * 2), ("bin_hist", C.c_size_t),
        ("bin_sorted", C.c_size_t), ("bin_work", C.c_size_t), ("bin_mask", C.c_size_t), ("bin_ckpt", C.c_size_t),
        ("bin_total", C.c_size_t), ("bin_lean_total", C.c_size_t), ("bin_staged", C.c_size_t),
        ("geom_vis_rec", C.c_size_t),  # ABI v9
    ]


class FrameInfo(C.Structure):
    _fields_ = [("num_rendered", C.c_int64), ("max_tile_instances", C.c_int64)]


ABI_VERSION = 9
BACKWARD_IMAGE_ONLY = 2  # gcr_camera.backward: an inference frame whose per-pixel state is not written either (include/gcr.h)
TICKET_WORDS = 8  # 64-bit pinned host words per asynchronous frame (include/gcr.h, gcr_forward_async)
RESIZE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_vp, _sz, _i32, _i64, _u32, _int = C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_uint32, C.c_int
_cam, _gs, _info, _opts = C.POINTER(Camera), C.POINTER(Gaussians), C.POINTER(FrameInfo), C.POINTER(Options)
# Every function include/gcr.h declares: name -> (restype, argtypes).  Tests hold this table to the header and to the
# symbols the built library exports.
_SIGNATURES = {
    "gcr_abi_version": (_int, []),
    "gcr_last_error": (C.c_char_p, []),
    "gcr_geometry_bytes": (_sz, [_i32]),
    "gcr_image_bytes": (_sz, [_i32, _i32]),
    "gcr_binning_bytes": (_sz, [_i64, _i32, _i32]),
    "gcr_binning_bytes_lean": (_sz, [_i64, _i32, _i32]),
    "gcr_get_layout": (_int, [_i32, _i32, _i32, _i64, C.POINTER(Layout)]),
    "gcr_forward": (_int, [_cam, _gs, _vp, _sz, _vp, _sz, _i64, _i64, _vp, _sz, _vp, _vp, _info, _vp]),
    "gcr_forward_preprocess": (_int, [_cam, _gs, _vp, _sz, _vp, _sz, _vp, _info, _vp]),
    "gcr_forward_render": (_int, [_cam, _gs, _vp, _sz, _vp, _sz, _vp, _sz, _info, _vp, _vp]),
    "gcr_backward": (_int, [_cam, _gs, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _i64, _vp, C.POINTER(Grads), _vp]),
    "gcr_build_cull_cache": (_int, [_gs, C.c_float, _vp, _vp]),
    "gcr_cull_cache_bytes": (_sz, [_i32]),
    "gcr_mark_visible": (_int, [_i32, _vp, _vp, _vp, _vp, _vp]),
    "gcr_rasterize_forward": (_i64, [RESIZE_FN, _vp, RESIZE_FN, _vp, RESIZE_FN, _vp, _cam, _gs, _vp, _vp, _vp]),
    "gcr_set_option": (_int, [C.c_char_p, _int]),
    "gcr_get_option": (_int, [C.c_char_p]),
    "gcr_get_stage_ms": (_int, [C.POINTER(C.c_float), _int]),
    "gcr_grad_record_floats": (_int, []),
    "gcr_grad_record_floats_opt": (_int, [_opts]),
    "gcr_forward_async": (_int, [_cam, _gs, _vp, _sz, _vp, _sz, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _u32, _vp]),
    "gcr_ticket_poll": (_int, [_vp, _u32, _i64, _info]),
    "gcr_ticket_wait": (_int, [_vp, _u32, _i64, _vp, _info]),
    "gcr_host_words_alloc": (_vp, [_sz]),
    "gcr_host_words_free": (None, [_vp]),
    "gcr_rescue_count": (C.c_long, []),
    "gcr_rescue_dropped_count": (C.c_long, []),
}


def _check_grad_record(L):
    if L.gcr_grad_record_floats() not in (GRAD_REC_FLOATS, 2 * GRAD_REC_FLOATS):
        raise RuntimeError("libgcr_hip.so gradient record size mismatch")


# GCR_LIB_PATH: tools/ point it at the experiment build (make -C csrc experiments); nothing else sets it
_L = _loader.Library("gcr", "libgcr_hip.so", ABI_VERSION, _SIGNATURES, STAGE_NAMES, path_env="GCR_LIB_PATH",
                     after_load=_check_grad_record)
LIB_PATH, EXPORTED_SYMBOLS = _L.path, _L.exported_symbols
lib, check, set_option, stage_ms = _L.lib, _L.check, _L.set_option, _L.stage_ms


def build(force=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", _loader.CSRC, "-s", "-j4"]
    if force:
        subprocess.check_call(["make", "-C", _loader.CSRC, "-s", "clean"])
    subprocess.check_call(cmd)
    return LIB_PATH


def get_layout(P, W, H, R):
    out = Layout()
    check(lib().gcr_get_layout(int(P), int(W), int(H), int(R), C.byref(out)), "gcr_get_layout")
    return out


def get_option(name):
    """Current process-wide default of a gcr_set_option() option (gcr_get_option, ABI v7: a plain read, safe beside other
    threads' frames).  Per-call values travel in gcr_options (ext.options), not here."""
    v = lib().gcr_get_option(name.encode())
    if v == -2 ** 31:
        raise KeyError("unknown rasterizer option %r" % name)
    return v
