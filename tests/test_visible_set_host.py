"""Visible point set (include/gcv.h K16, ABI v5), the part that needs no GPU: the three new entry points are exported
and bound, the workspace size query, the argument checks that come back before any HIP call, the Python layer's centers
table and class-rule presets, and the numpy reference itself on a case whose expected arrays are written out here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gaussiancity_amd import _native_v as V
from gaussiancity_amd import points as P
from visible_ref import visible_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_SMALL = -1, -4


def test_new_symbols_are_exported_and_abi_is_5():
    lib = V.lib()
    for name in ("gcv_visible_workspace_bytes", "gcv_visible_count", "gcv_visible_emit"):
        assert name in V.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "gcv.h")).read()
    assert lib.gcv_abi_version() == 5 == V.ABI_VERSION == int(re.search(r"#define GCV_ABI_VERSION (\d+)", header).group(1))
    assert V.STAGE_NAMES[:6] == ("extrude_count", "extrude_emit", "volume_clear", "volume_scatter", "occupancy", "traversal")
    assert V.STAGE_NAMES[6:] == ("visible_count", "visible_emit")
    assert C.sizeof(V.ClassRule) == 32


def test_workspace_bytes_positive_monotone_and_range_checked():
    lib = V.lib()
    sizes = [lib.gcv_visible_workspace_bytes(n, 960 * 540) for n in (0, 1, 31, 32, 33, 100_003, 17_300_000, 2 ** 31 - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[6] >= 17_300_000 // 8 and sizes[6] < 4 * 17_300_000 // 8   # a bitmap over the points, not a list
    for n, npix in ((-1, 10), (10, -1), (2 ** 31, 10), (2 ** 40, 10)):
        lib.gcv_visible_count(None, 0, None, 0, None, 0, None, 0, None, None)   # (some other error text first)
        assert lib.gcv_visible_workspace_bytes(n, npix) == 0
        assert b"gcv_visible_workspace_bytes" in lib.gcv_last_error()


def _host_args():
    """Host memory in the roles of the device buffers: every call below fails a check before anything is read."""
    buf = (C.c_double * 4096)()
    p = (C.addressof(buf) + 255) // 256 * 256
    return buf, p


def test_count_argument_errors_come_back_before_any_hip_call():
    lib = V.lib()
    buf, p = _host_args()
    counts = (C.c_int64 * 3)(-7, -7, -7)
    need = lib.gcv_visible_workspace_bytes(1000, 64)

    def call(vp=p, npix=64, rows=p, n=1000, cen=p, nc=4, ws=p, wsb=need, out=counts):
        return lib.gcv_visible_count(vp, npix, rows, n, cen, nc, ws, wsb, out, None)

    for kw in (dict(vp=None), dict(rows=None), dict(cen=None), dict(ws=None), dict(out=None)):
        assert call(**kw) == INVALID and b"null" in lib.gcv_last_error(), kw
    for kw in (dict(npix=-1), dict(n=-1), dict(nc=-1), dict(n=2 ** 31), dict(npix=2 ** 31)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(vp=p + 4), dict(rows=p + 1), dict(cen=p + 4), dict(ws=p + 8)):
        assert call(**kw) == INVALID and b"misaligned" in lib.gcv_last_error(), kw
    assert call(wsb=need - 1) == TOO_SMALL and b"workspace too small" in lib.gcv_last_error()
    assert call(wsb=0) == TOO_SMALL
    assert list(counts) == [-7, -7, -7]
    with pytest.raises(RuntimeError, match="gcv_status -4"):
        V.check(call(wsb=8), "gcv_visible_count")


def test_emit_argument_errors_come_back_before_any_hip_call():
    lib = V.lib()
    buf, p = _host_args()
    rule = V.ClassRule(100, 0, 0, 2, 7, 0, 0b1100010, 0.45)
    need = lib.gcv_visible_workspace_bytes(1000, 64)

    def call(vp=p, npix=64, rows=p, n=1000, cen=p, nc=4, r=C.byref(rule), ws=p, wsb=need, m=10, k=2, index=p, pts=p,
             batch=p, ins=p, cls=p, sc=p):
        return lib.gcv_visible_emit(vp, npix, rows, n, cen, nc, r, ws, wsb, m, k, index, pts, batch, ins, cls, sc, None)

    for kw in (dict(vp=None), dict(rows=None), dict(cen=None), dict(ws=None), dict(r=None), dict(index=None), dict(pts=None)):
        assert call(**kw) == INVALID and b"null" in lib.gcv_last_error(), kw
    for kw in (dict(npix=-1), dict(n=-1), dict(nc=-1), dict(m=-1), dict(k=-1), dict(m=1001), dict(k=11)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(index=p + 4), dict(pts=p + 8), dict(batch=p + 2), dict(ins=p + 1), dict(cls=p + 2), dict(sc=p + 2)):
        assert call(**kw) == INVALID and b"misaligned" in lib.gcv_last_error(), kw
    assert call(wsb=need - 1) == TOO_SMALL
    assert call(m=0, k=0, index=None, pts=None) == 0      # nothing visible: nothing to enqueue


def test_centers_table_nan_padding_cache_and_rebuild():
    centers = {3: (1.5, 2.5, 4.0, 6.0, 8.0), 0: (0.0, 0.0, 0.0, 0.0, 0.0), np.int16(5): np.array([9.0, 8.0, 7.0, 6.0, 5.0])}
    t = P.centers_table(centers)
    assert t.dtype.is_floating_point and t.element_size() == 8 and tuple(t.shape) == (6, 5)
    a = t.numpy()
    assert np.array_equal(a[3], [1.5, 2.5, 4.0, 6.0, 8.0]) and np.array_equal(a[0], np.zeros(5)) and np.array_equal(a[5], [9, 8, 7, 6, 5])
    assert np.isnan(a[[1, 2, 4]]).all()
    assert P.centers_table(centers) is t                      # cached on the dict's id and length
    centers[9] = (1.0, 1.0, 1.0, 1.0, 1.0)
    t2 = P.centers_table(centers)
    assert t2 is not t and tuple(t2.shape) == (10, 5) and np.array_equal(t2.numpy()[9], np.ones(5))
    assert np.isnan(t2.numpy()[[6, 7, 8]]).all() and P.centers_table(centers) is t2
    assert tuple(P.centers_table({}).shape) == (0, 5)
    for bad in ({-1: (0, 0, 1, 1, 1)}, {32768: (0, 0, 1, 1, 1)}):
        with pytest.raises(KeyError):
            P.centers_table(bad)


def test_class_rule_presets_are_the_reference_constants():
    ge, ki = P.CLASS_RULE_GOOGLE_EARTH, P.CLASS_RULE_KITTI_360
    assert tuple(ge) == (100, 0, 0, 2, 7, 0, (1, 5, 6), 0.45)
    assert tuple(ki) == (100, 10000, 10000, 2, 7, 3, (1, 6), 0.5)
    n = P._native_rule(ge)
    assert (n.bldg_ins_min, n.bldg_ins_max, n.car_ins_min, n.facade_class, n.roof_class, n.car_class) == (100, 0, 0, 2, 7, 0)
    assert n.special_z_classes == (1 << 1) | (1 << 5) | (1 << 6) and n.point_scale_factor == np.float32(0.45)
    n = P._native_rule(ki, point_scale_factor=0.25)
    assert n.special_z_classes == (1 << 1) | (1 << 6) and n.point_scale_factor == 0.25 and n.car_class == 3
    with pytest.raises(ValueError):
        P._native_rule(ge._replace(special_z_classes=(40,)))


def test_reference_on_a_hand_written_case():
    rows = np.array([[10, 20, 0, 2, 1],      # road
                     [12, 20, 0, 2, 1],      # road, never seen
                     [30, 40, 5, 1, 100],    # facade of building 100
                     [30, 40, 10, 1, 101],   # its roof
                     [31, 40, 50, 1, 100],   # facade, above the box: z clips to 1
                     [7, 7, 0, 4, 5]], np.int16)   # water, never seen
    vp_map = np.array([[3, -1, 0, 3], [4, 2, -1, 0]], np.int64)
    centers = {1: (0.0, 0.0, 0.0, 0.0, 0.0), 100: (32.0, 44.0, 8.0, 16.0, 20.0), 101: (32.0, 44.0, 8.0, 16.0, 20.0)}
    r = visible_ref(rows, vp_map, centers, P.CLASS_RULE_GOOGLE_EARTH)
    assert r["index"].tolist() == [0, 2, 3, 4] and r["index"].dtype == np.int64
    assert r["instances"].tolist() == [1, 100, 101] and r["instances"].dtype == np.int16
    assert r["batch_idx"].tolist() == [0, 1, 2, 1] and r["batch_idx"].dtype == np.int32
    want = np.array([[10, 20, 0, 2, 1, 0.0, 0.0, 0.0],
                     [30, 40, 5, 1, 100, -0.5, -0.5, -0.5],
                     [30, 40, 10, 1, 101, -0.5, -0.5, 0.0],
                     [31, 40, 50, 1, 100, -0.25, -0.5, 1.0]], np.float32)
    assert r["pts"].dtype == np.float32 and np.array_equal(r["pts"], want)
    assert r["classes"].tolist() == [1.0, 2.0, 7.0, 2.0]
    s2, s1 = np.float32(2) * np.float32(0.45), np.float32(0.45)
    assert r["scales"].dtype == np.float32 and np.array_equal(r["scales"], np.array([[s2, s2, 1.0], [s1, s1, s1], [s1, s1, s1],
                                                                                     [s1, s1, s1]], np.float32))
    # KITTI-360: 100 and 101 are still buildings, the factor is 0.5; an id from 10000 on is a car
    k = visible_ref(rows, vp_map, centers, P.CLASS_RULE_KITTI_360)
    assert k["classes"].tolist() == [1.0, 2.0, 7.0, 2.0] and k["scales"][:, 0].tolist() == [1.0, 0.5, 0.5, 0.5]
    rows[4, 4] = 10000
    with pytest.raises(KeyError):
        visible_ref(rows, vp_map, centers, P.CLASS_RULE_KITTI_360)
    centers[10000] = (0.0, 0.0, 1.0, 1.0, 1.0)
    assert visible_ref(rows, vp_map, centers, P.CLASS_RULE_KITTI_360)["classes"].tolist() == [1.0, 2.0, 7.0, 3.0]
    # the NaN-padded table means the same as the dict
    t = visible_ref(rows, vp_map, P.centers_table(centers).numpy(), P.CLASS_RULE_KITTI_360)
    assert all(np.array_equal(t[key], v) for key, v in visible_ref(rows, vp_map, centers, P.CLASS_RULE_KITTI_360).items())
