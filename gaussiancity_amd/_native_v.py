"""ctypes binding of libgcv_hip.so (C ABI in include/gcv.h): point generation / visibility path.  The declarations;
gaussiancity_amd/_loader.py loads it.

The library is the product: there is NO Python/CPU fallback -- a missing library or a failing call
raises RuntimeError.
"""
import ctypes as C

from . import _loader

STAGE_NAMES = ("extrude_count", "extrude_emit", "volume_clear", "volume_scatter", "occupancy", "traversal",
               "visible_count", "visible_emit")
ABI_VERSION = 5


class SegIns(C.Structure):
    """gcv_seg_ins == segInsMap (footprint_extruder.cpp:90-100,201)."""
    _fields_ = [(n, C.c_int16) for n in ("bldg_ins_min_id", "car_ins_min_id", "car_semantic_id",
                                         "bldg_facade_semantic_id", "roof_ins_offset")]


class ClassRule(C.Structure):
    """gcv_class_rule: instance id -> class and z-scale (scripts/inference.py:544-598, utils/helpers.py:212-222)."""
    _fields_ = [(n, C.c_int32) for n in ("bldg_ins_min", "bldg_ins_max", "car_ins_min", "facade_class", "roof_class",
                                         "car_class")] + [("special_z_classes", C.c_uint32),
                                                          ("point_scale_factor", C.c_float)]


class ModelRule(C.Structure):
    """gcv_model_rule: class -> model slot (0 BLDG, 1 CAR, 2 REST, -1 dropped; scripts/inference.py:426-452) and the
    constants of get_projection_uv (utils/helpers.py:183-194)."""
    _fields_ = [("n_classes", C.c_int32), ("model_of_class", C.c_int8 * 32), ("proj_tlp", C.c_float * 2),
                ("proj_size", C.c_float)]


class GaussianSegment(C.Structure):
    """gcv_gaussian_segment: one model's rows and the generator's outputs for them (NULL = the key is absent)."""
    _fields_ = [("n", C.c_int64)] + [(n, C.c_void_p) for n in ("rgb", "dxyz", "scale", "opacity")]


class GaussianAttrs(C.Structure):
    """gcv_gaussian_attrs: up to three segments, passed by value."""
    _fields_ = [("n_segments", C.c_int32), ("seg", GaussianSegment * 3)]


class TrainRule(C.Structure):
    """gcv_train_rule: instance id -> class, the one-hot's width, the special z classes and the constants of
    get_point_scales' caller and get_projection_uv (core/train.py:207-224)."""
    _fields_ = [(n, C.c_int32) for n in ("bldg_ins_min", "bldg_ins_max", "car_ins_min", "car_ins_max", "facade_class",
                                         "roof_class", "car_class", "n_classes")] + [
        ("special_z_classes", C.c_uint32), ("scale_factor", C.c_float), ("proj_size", C.c_float)]


TRAIN_INPUTS_FLAG_OFFSET = 8  # GCV_TRAIN_INPUTS_FLAG_OFFSET: the flag word's byte offset in the workspace

_vp, _i32, _i64, _sz, _f32, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float, C.c_int
_pi32, _pf32, _seg = C.POINTER(_i32), C.POINTER(_f32), C.POINTER(SegIns)
_st3, _st2 = C.POINTER(_i64 * 3), C.POINTER(_i64 * 2)  # HOST element strides {batch, channel, row} / {batch, row}
_SIGNATURES = {  # every function include/gcv.h declares: name -> (restype, argtypes)
    "gcv_abi_version": (_int, []),
    "gcv_last_error": (C.c_char_p, []),
    "gcv_extrude_scratch_bytes": (_sz, [_i32, _i32]),
    "gcv_extrude_count": (_int, [_i32, _vp, _seg, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_i64), _vp]),
    "gcv_extrude_emit": (_int, [_i32, _vp, _seg, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _i64, _vp]),
    "gcv_maps_to_volume": (_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "gcv_occupancy_bytes": (_sz, [_i32, _i32, _i32]),
    "gcv_points_to_volume": (_int, [_i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "gcv_build_occupancy": (_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "gcv_bounds_scratch_bytes": (_sz, []),
    "gcv_points_bounds": (_int, [_i64, _vp, _i32, _vp, _pi32, _pi32, _vp]),
    "gcv_rows_to_volume": (_int, [_i64, _vp, _pi32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "gcv_rows_erase_volume": (_int, [_i64, _vp, _pi32, _i32, _i32, _i32, _vp, _vp]),
    "gcv_ray_voxel_intersection": (_int, [_vp, _pi32, C.POINTER(_i64), _vp, _pf32, _pf32, _pf32, _f32, _pf32, _pi32, _i32,
                                          _vp, _vp, _vp, _vp]),
    "gcv_visible_workspace_bytes": (_sz, [_i64, _i64]),
    "gcv_visible_count": (_int, [_vp, _i64, _vp, _i64, _vp, _i32, _vp, _sz, C.POINTER(_i64), _vp]),
    "gcv_visible_emit": (_int, [_vp, _i64, _vp, _i64, _vp, _i32, C.POINTER(ClassRule), _vp, _sz, _i64, _i64,
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gcv_model_split_models": (_int, []),
    "gcv_model_split_workspace_bytes": (_sz, [_i64, _i64]),
    "gcv_model_split_count": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i32, C.POINTER(ModelRule), _vp, _sz,
                                     C.POINTER(_i64), _vp]),
    "gcv_model_split_emit": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, C.POINTER(ModelRule), _vp,
                                    _sz, C.POINTER(_i64)] + [_vp] * 11),
    "gcv_gaussian_points": (_int, [_vp, _i64, _vp, _i64, _i64, GaussianAttrs, _vp, _vp]),
    "gcv_frame_finish_radius_max": (_int, []),
    "gcv_frame_finish": (_int, [_vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _pf32, _vp, _vp, _i32, _vp]),
    "gcv_image_loss_max_classes": (_int, []),
    "gcv_image_loss_partials": (_i64, [_i64, _i32]),
    "gcv_mean_abs_forward": (_int, [_vp, _st3, _vp, _st3, _vp, _st2, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "gcv_mean_abs_backward": (_int, [_vp, _st3, _vp, _st3, _vp, _st2, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "gcv_gan_loss_forward": (_int, [_vp, _st3, _vp, _st3, _vp, _st2, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "gcv_gan_loss_backward": (_int, [_vp, _st3, _vp, _st3, _vp, _st2, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "gcv_label_map": (_int, [_vp, _st3, _vp, _st2, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "gcv_train_inputs_max_classes": (_int, []),
    "gcv_train_inputs_workspace_bytes": (_sz, [_i64]),
    "gcv_train_inputs_count": (_int, [_vp, _i64, _i64, _vp, _sz, C.POINTER(_i64), _vp]),
    "gcv_train_inputs_emit": (_int, [_vp, _i64, _i64, _i64, C.POINTER(TrainRule), _vp, _vp, _sz, _i32, _i64] + [_vp] * 8),
    "gcv_set_option": (_int, [C.c_char_p, _int]),
    "gcv_get_stage_ms": (_int, [_pf32, _int]),
}

_L = _loader.Library("gcv", "libgcv_hip.so", ABI_VERSION, _SIGNATURES, STAGE_NAMES)
LIB_PATH, EXPORTED_SYMBOLS = _L.path, _L.exported_symbols
lib, check, set_option, stage_ms = _L.lib, _L.check, _L.set_option, _L.stage_ms
