"""Per-model generator inputs (include/gcv.h K17, K18; gaussiancity_amd.model_inputs), the part that needs no GPU: the
numpy formulation against the recorded reference, the header / binding / export lists, the probe, the argument checks
that come back before any HIP call, the workspace size query, GroupedCodes and StyleTable on CPU tensors, the rule
presets."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gaussiancity_amd import _native_v as V
from gaussiancity_amd import model_inputs as MI
import model_inputs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_inputs.npz")
INVALID, TOO_SMALL = -1, -4
NEW = ("gcv_model_split_models", "gcv_model_split_workspace_bytes", "gcv_model_split_count", "gcv_model_split_emit",
       "gcv_gaussian_points")


@pytest.fixture(scope="module")
def cases():
    return R.golden_cases(GOLDEN)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(R.bits(got), R.bits(want)), what


def test_golden_covers_what_it_should(cases):
    assert {str(c["dataset"]) for c in cases.values()} == {"GOOGLE_EARTH", "KITTI_360"}
    assert any(c["tlp"].size for c in cases.values()) and any(not c["tlp"].size for c in cases.values())
    assert any(int(c["proj_size"]) & (int(c["proj_size"]) - 1) for c in cases.values())            # not a power of two
    assert any(bool(c[k + "/called"]) and bool(c[k + "/zs_is_none"]) for c in cases.values() for k in R.MODELS)
    assert any(not c["present"][2] for c in cases.values()) and any(bool(c["CAR/called"]) for c in cases.values())
    for c in cases.values():                              # a LUT that lacks visible instances, and ids nobody sees
        assert not set(c["lut_ids"].tolist()) >= set(c["instances"].tolist())
    some = cases["ge_all"]
    keys, ids = some["BLDG/zs_keys"].tolist(), some["instances"].tolist()
    assert keys == sorted(keys) and any(i not in keys for i in ids if keys[0] < i < keys[-1])     # a gap in the middle
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_numpy_formulation_reproduces_the_recorded_reference_bit_for_bit(cases):
    for name, c in cases.items():
        ref = R.model_inputs_ref(**R.golden_inputs(c))
        attrs = {}
        for k in R.MODELS:
            assert bool(c[k + "/called"]) == (k in ref["models"]), (name, k)
            if k not in ref["models"]:
                continue
            m = ref["models"][k]
            assert np.array_equal(np.nonzero(c[k + "/mask"])[0], m["index"]), (name, k)
            _same(m["proj_uv"][None], c[k + "/proj_uv"], (name, k, "proj_uv"))
            _same(m["rel_xyz"][None], c[k + "/rel_xyz"], (name, k, "rel_xyz"))
            _same(m["batch_idx"][None], c[k + "/batch_idx"], (name, k, "batch_idx"))
            _same(m["onehots"][None], c[k + "/onehots"], (name, k, "onehots"))
            assert bool(c[k + "/zs_is_none"]) == (m["zs"] is None), (name, k)
            if m["zs"] is not None:
                assert list(m["zs"]) == c[k + "/zs_keys"].tolist(), (name, k)
                _same(m["codes"], c[k + "/zs_z"], (name, k, "codes"))
                _same(np.concatenate([v["idx"] for v in m["zs"].values()]), c[k + "/zs_idx"], (name, k, "idx"))
                assert np.array_equal(m["group_instances"], c[k + "/zs_keys"]) and m["group"].max() == len(m["zs"]) - 1
            for a in c["keys"]:
                attrs.setdefault(str(a), []).append(c[k + "/attr_" + str(a)][0])
        _same(ref["abs_xyz"][None], c["abs_xyz"], (name, "abs_xyz"))
        _same(ref["scales"][None], c["cat_scales"], (name, "scales"))
        cat = {a: np.concatenate(v) for a, v in attrs.items()}
        for a, v in cat.items():
            _same(v[None], c["cat_" + a], (name, a))
        _same(R.gaussian_points_ref(ref["abs_xyz"], ref["scales"], cat)[None], c["gs_pts"], (name, "gs_pts"))


def test_header_binding_and_exports_agree():
    header = open(os.path.join(ROOT, "include", "gcv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gcv_[a-z0-9_]+)\s*\(", code))
    assert declared == set(V.EXPORTED_SYMBOLS) and set(NEW) <= declared
    lib = V.lib()
    for name in declared:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.gcv_model_split_models() == 3 == len(MI.MODELS)
    assert lib.gcv_abi_version() == 5 == V.ABI_VERSION == int(re.search(r"#define GCV_ABI_VERSION (\d+)", header).group(1))
    assert V.STAGE_NAMES[6:] == ("visible_count", "visible_emit")                 # the timers are as they were
    assert C.sizeof(V.ModelRule) == 48 and C.sizeof(V.GaussianSegment) == 40 and C.sizeof(V.GaussianAttrs) == 128


def test_workspace_bytes_range_checked_and_monotone():
    lib = V.lib()
    sizes = [lib.gcv_model_split_workspace_bytes(m, 60) for m in (0, 1, 256, 257, 160_000, 2 ** 31 - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[4] < 160_000                              # three counters per block of rows, not a word per row
    assert lib.gcv_model_split_workspace_bytes(1000, 65536) > lib.gcv_model_split_workspace_bytes(1000, 1)
    for m, k in ((-1, 10), (10, -1), (2 ** 31, 10), (2 ** 40, 10), (10, 65537)):
        lib.gcv_visible_count(None, 0, None, 0, None, 0, None, 0, None, None)     # (some other error text first)
        assert lib.gcv_model_split_workspace_bytes(m, k) == 0
        assert b"gcv_model_split_workspace_bytes" in lib.gcv_last_error()


def _host_args():
    """Host memory in the roles of the device buffers: every call below fails a check before anything is read."""
    buf = (C.c_double * 4096)()
    return buf, (C.addressof(buf) + 255) // 256 * 256


def _rule(**kw):
    r = MI._native_rule(MI.MODEL_RULE_KITTI_360(), None, 2048)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_count_argument_errors_come_back_before_any_hip_call():
    lib = V.lib()
    buf, p = _host_args()
    counts = (C.c_int64 * 9)(*[-7] * 9)
    need = lib.gcv_model_split_workspace_bytes(1000, 40)
    rule = _rule()

    def call(cls=p, bi=p, m=1000, ins=p, k=40, has=p, n_lut=50, r=C.byref(rule), ws=p, wsb=need, out=counts):
        return lib.gcv_model_split_count(cls, bi, m, ins, k, has, n_lut, r, ws, wsb, out, None)

    for kw in (dict(cls=None), dict(bi=None), dict(ins=None), dict(has=None), dict(r=None), dict(ws=None), dict(out=None)):
        assert call(**kw) == INVALID and b"null" in lib.gcv_last_error(), kw
    for kw in (dict(m=-1), dict(k=-1), dict(n_lut=-1), dict(m=2 ** 31), dict(k=65537)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(cls=p + 2), dict(bi=p + 2), dict(ins=p + 1), dict(ws=p + 8)):
        assert call(**kw) == INVALID and b"misaligned" in lib.gcv_last_error(), kw
    for bad in (_rule(n_classes=0), _rule(n_classes=33), _rule(proj_size=0.0), _rule(proj_size=float("nan"))):
        assert call(r=C.byref(bad)) == INVALID, bad
    bad = _rule()
    bad.model_of_class[3] = 3
    assert call(r=C.byref(bad)) == INVALID and b"model_of_class" in lib.gcv_last_error()
    bad.model_of_class[3] = -2
    assert call(r=C.byref(bad)) == INVALID
    assert call(wsb=need - 1) == TOO_SMALL and b"workspace too small" in lib.gcv_last_error()
    assert call(wsb=0) == TOO_SMALL
    assert list(counts) == [-7] * 9
    with pytest.raises(RuntimeError, match="gcv_status -4"):
        V.check(call(wsb=8), "gcv_model_split_count")


def test_emit_argument_errors_come_back_before_any_hip_call():
    lib = V.lib()
    buf, p = _host_args()
    need = lib.gcv_model_split_workspace_bytes(1000, 40)
    rule = _rule()
    good = (C.c_int64 * 9)(600, 100, 300, 20, 5, 15, 10, 0, 3)

    def call(cls=p, bi=p, p8=p, sc=p, m=1000, ins=p, k=40, has=p, lut=p, n_lut=50, z=8, r=C.byref(rule), ws=p, wsb=need,
             cnt=good, outs=None, **named):
        o = dict.fromkeys(("index", "pts", "batch", "classes", "scales", "onehots", "uv", "group", "gins", "codes"), p)
        o.update(named)
        return lib.gcv_model_split_emit(cls, bi, p8, sc, m, ins, k, has, lut, n_lut, z, r, ws, wsb, cnt, *o.values(), None)

    for kw in (dict(cls=None), dict(bi=None), dict(ins=None), dict(has=None), dict(r=None), dict(ws=None), dict(cnt=None),
               dict(p8=None), dict(sc=None), dict(lut=None)):
        assert call(**kw) == INVALID and b"null" in lib.gcv_last_error(), kw
    for kw in (dict(m=-1), dict(k=-1), dict(n_lut=-1), dict(z=-1), dict(m=2 ** 31), dict(k=65537)):
        assert call(**kw) == INVALID, kw
    for bad in ((-1, 0, 0, 0, 0, 0, 0, 0, 0), (600, 100, 301, 20, 5, 15, 10, 0, 3), (600, 100, 300, 41, 5, 15, 10, 0, 3),
                (600, 100, 300, 20, 5, 15, 21, 0, 3), (600, 100, 300, 20, 5, 15, 10, 0, -1), (4, 0, 0, 5, 0, 0, 0, 0, 0)):
        assert call(cnt=(C.c_int64 * 9)(*bad)) == INVALID and b"counts" in lib.gcv_last_error() or b"exceeds" in lib.gcv_last_error(), bad
    for kw in (dict(p8=p + 8), dict(sc=p + 2), dict(lut=p + 2), dict(index=p + 4), dict(pts=p + 8), dict(batch=p + 2),
               dict(classes=p + 2), dict(scales=p + 2), dict(onehots=p + 2), dict(uv=p + 2), dict(group=p + 2),
               dict(gins=p + 1), dict(codes=p + 2)):
        assert call(**kw) == INVALID and b"misaligned" in lib.gcv_last_error(), kw
    assert call(wsb=need - 1) == TOO_SMALL
    assert call(cnt=(C.c_int64 * 9)(), p8=None, sc=None, lut=None) == 0        # no rows: nothing to enqueue


def test_points14_argument_errors_come_back_before_any_hip_call():
    lib = V.lib()
    buf, p = _host_args()

    def rec(n_segments=2, sizes=(60, 40, 0), **ptrs):
        a = V.GaussianAttrs()
        a.n_segments = n_segments
        for i, n in enumerate(sizes):
            a.seg[i].n = n
            for key in ("rgb", "dxyz", "scale", "opacity"):
                setattr(a.seg[i], key, ptrs.get("%s%d" % (key, i), p if n else None))
        return a

    def call(xyz=p, xs=8, sc=p, ss=3, n=100, a=None, out=p):
        return lib.gcv_gaussian_points(xyz, xs, sc, ss, n, a if a is not None else rec(), out, None)

    for kw in (dict(xyz=None), dict(sc=None), dict(out=None), dict(a=rec(rgb1=None))):
        assert call(**kw) == INVALID and b"null" in lib.gcv_last_error(), kw
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(n=99), dict(xs=2), dict(ss=0), dict(a=rec(n_segments=0)), dict(a=rec(n_segments=4)),
               dict(a=rec(sizes=(110, -10, 0)))):
        assert call(**kw) == INVALID, kw
    for key in ("dxyz", "scale", "opacity"):                 # a key in one model's dict and not in the other's
        assert call(a=rec(**{key + "1": None})) == INVALID and b"every segment or in none" in lib.gcv_last_error(), key
    for kw in (dict(xyz=p + 2), dict(sc=p + 2), dict(out=p + 4), dict(a=rec(rgb0=p + 2)), dict(a=rec(opacity1=p + 1))):
        assert call(**kw) == INVALID and b"misaligned" in lib.gcv_last_error(), kw
    assert call(n=0, a=rec(sizes=(0, 0, 0)), xyz=None, sc=None, out=None) == 0     # no rows: nothing to enqueue


def test_grouped_codes_stands_for_the_dict(cases):
    c = cases["ge_all"]
    ref = R.model_inputs_ref(**R.golden_inputs(c))["models"]["BLDG"]
    zs = MI.GroupedCodes(torch.from_numpy(ref["group"]), torch.from_numpy(ref["codes"]), torch.from_numpy(ref["group_instances"]))
    want = ref["zs"]
    assert len(zs) == len(want) >= 3 and list(zs) == list(want) == zs.keys() and (-1 in ref["group"])
    assert not isinstance(zs, dict) and list(want)[1] in zs and 5 not in zs
    for (ui, v), w, (uk, item) in zip(want.items(), zs.values(), zs.items()):
        assert uk == ui
        for e in (w, item, zs[ui]):
            assert e["z"].shape == (1, ref["codes"].shape[1]) and e["idx"].dtype == torch.bool and e["idx"].shape == (1, len(ref["group"]))
            assert np.array_equal(R.bits(e["z"].numpy()), R.bits(v["z"])) and np.array_equal(e["idx"].numpy(), v["idx"])
        assert w["z"].data_ptr() == zs.codes[list(want).index(ui)].data_ptr()        # a view of the table, not a copy
    with pytest.raises(KeyError):
        zs[5]
    with pytest.raises(TypeError):
        zs[5] = {"z": None}
    with pytest.raises(TypeError):
        del zs[list(want)[0]]
    with pytest.raises(TypeError):
        zs.group = None
    with pytest.raises(TypeError):
        del zs.codes
    # DataParallel's scatter copies dicts, lists and tuples; anything else goes through as the same object
    from torch.nn.parallel.scatter_gather import scatter_kwargs
    _, kw = scatter_kwargs((), {"zs": zs}, [0]) if torch.cuda.is_available() else ((), ({"zs": zs},))
    assert kw[0]["zs"] is zs


def test_style_table_ragged_widths_missing_ids_and_cache():
    lut = {3: torch.arange(4.0).reshape(1, 4), 0: torch.ones(1, 4), np.int16(6): torch.full((1, 4), 2.0)}
    t = MI.StyleTable(lut, "cpu")
    assert (t.n_lut, t.z_dim) == (7, 4) and t.lut.dtype == torch.float32 and t.lut_has.dtype == torch.uint8
    assert t.lut_has.tolist() == [1, 0, 0, 1, 0, 0, 1] and t.lut[3].tolist() == [0, 1, 2, 3] and t.lut[6].tolist() == [2] * 4
    assert t.lut[[1, 2, 4, 5]].abs().sum() == 0
    with pytest.raises(ValueError, match="one width"):
        MI.StyleTable({1: torch.zeros(1, 4), 2: torch.zeros(1, 5)}, "cpu")
    for bad in ({-1: torch.zeros(1, 4)}, {32768: torch.zeros(1, 4)}):
        with pytest.raises(KeyError):
            MI.StyleTable(bad, "cpu")
    e = MI.StyleTable({}, "cpu")
    assert (e.n_lut, e.z_dim) == (0, 0)
    assert MI.style_table(lut, "cpu") is MI.style_table(lut, "cpu")              # cached on the dict's id and length
    first = MI.style_table(lut, "cpu")
    lut[9] = torch.zeros(1, 4)
    assert MI.style_table(lut, "cpu") is not first and MI.style_table(lut, "cpu").n_lut == 10


def test_rule_presets_and_tlp_conversion():
    for ds, make in (("GOOGLE_EARTH", MI.MODEL_RULE_GOOGLE_EARTH), ("KITTI_360", MI.MODEL_RULE_KITTI_360)):
        for bldg in (True, False):
            for car in ((True, False) if ds == "KITTI_360" else (False,)):
                rule = make(bldg, car) if ds == "KITTI_360" else make(bldg)
                want = R.model_of_class(R.CLASS_IDS[ds], 8, bldg, car, True)
                assert rule.n_classes == 8 and list(rule.model_of_class) == want[:8].tolist(), (ds, bldg, car)
                n = MI._native_rule(rule, None, 2048)
                assert list(n.model_of_class) == want.tolist() and tuple(n.proj_tlp) == (0.0, 0.0) and n.proj_size == 2048.0
    assert list(MI.MODEL_RULE_KITTI_360(rest=False).model_of_class) == [-1, -1, 0, 1, -1, -1, -1, 0]
    assert list(MI.MODEL_RULE_GOOGLE_EARTH(bldg=False).model_of_class) == [2] * 8
    n = MI._native_rule(MI.MODEL_RULE_GOOGLE_EARTH(), np.array([16777217, -3]), 1000)      # int64 -> float32, rounded as torch does
    assert tuple(n.proj_tlp) == (16777216.0, -3.0) and n.proj_size == 1000.0
    assert tuple(MI._native_rule(MI.MODEL_RULE_GOOGLE_EARTH(), torch.tensor([[1.5, 2.5]]), 8).proj_tlp) == (1.5, 2.5)
    with pytest.raises(TypeError):
        MI._native_rule(MI.MODEL_RULE_GOOGLE_EARTH(), np.array([1.5, 2.5]), 8)             # float64: upstream would promote
    with pytest.raises(ValueError):
        MI._native_rule(MI.MODEL_RULE_GOOGLE_EARTH(), [1, 2, 3], 8)
    with pytest.raises(ValueError):
        MI._native_rule(MI.ModelRule(8, (0, 1, 2, 3, 0, 0, 0, 0)), None, 8)
    assert set(MI.stats()) == {"split_calls", "points14_calls"}
