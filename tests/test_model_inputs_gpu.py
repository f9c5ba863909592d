"""-m gpu: per-model generator inputs and the [N,14] assembly on the device (gaussiancity_amd.model_inputs ->
gcv_model_split_count / gcv_model_split_emit / gcv_gaussian_points -> gfx950 kernels), through the C ABI and through Python, against
the numpy formulation in model_inputs_ref.py (which tests/golden/model_inputs.npz holds to the reference's own lines).
Index work plus single-rounded fp32 operations, so the bar is BIT-EXACT for every output, dtypes and shapes as upstream's."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from gaussiancity_amd import _native_v as V
from gaussiancity_amd import helpers as H
from gaussiancity_amd import model_inputs as MI
from gaussiancity_amd import points as P
import model_inputs_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_inputs.npz")
BLOCK = 256                  # rows per block of the count / emit kernels
INVALID = -1
CANARY = 64                  # elements of canary on either side of every raw output
KITTI = R.model_of_class(R.CLASS_IDS["KITTI_360"], 8)


def _classes_of(ins):
    """KITTI-360's instance -> class rule (points.CLASS_RULE_KITTI_360), enough to give the rows three models."""
    ins = ins.astype(np.int64)
    cls = ins.copy()
    bldg = (ins >= 100) & (ins < 10000)
    cls[bldg & (ins % 2 == 0)], cls[bldg & (ins % 2 == 1)], cls[ins >= 10000] = 2, 7, 3
    return cls.astype(np.float32)


def _frame(rng, m, ids, first=None, last=None):
    """A visible set in numpy: rows of random instances out of `ids` (every id at least once when m allows)."""
    ids = np.sort(np.array(ids, np.int16))
    ins = ids[rng.integers(0, len(ids), m)]
    if m >= len(ids):
        ins[rng.permutation(m)[:len(ids)]] = ids
    if first is not None and m:
        ins[0] = first
    if last is not None and m:
        ins[-1] = last
    present = np.unique(ins)
    pts = np.empty((m, 8), np.float32)
    pts[:, :3] = rng.integers(-300, 2300, (m, 3))
    pts[:, 3] = rng.integers(1, 5, m)
    pts[:, 4] = ins
    pts[:, 5:] = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    return dict(pts=pts, batch_idx=np.searchsorted(present, ins).astype(np.int32), instances=present.astype(np.int16),
                classes=_classes_of(ins), scales=rng.uniform(0.4, 2.0, (m, 3)).astype(np.float32))


def _lut(rng, ids, z_dim=12):
    return {int(i): rng.uniform(-1, 1, z_dim).astype(np.float32) for i in ids}


def _visible_set(dev, f):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    m = len(f["pts"])
    return P.VisibleSet(torch.arange(m, device=dev), t(f["pts"]).reshape(1, m, 8), t(f["batch_idx"]).reshape(1, m, 1),
                        t(f["instances"]), t(f["classes"]).reshape(1, m, 1), t(f["scales"]).reshape(1, m, 3))


def _torch_lut(lut):
    return {i: torch.from_numpy(z)[None] for i, z in lut.items()}


def _same(got, want, what, dtype, shape):
    assert got.dtype == dtype and tuple(got.shape) == tuple(shape), (what, got.dtype, tuple(got.shape), shape)
    g = got.cpu().numpy().reshape(want.shape)
    assert g.dtype == want.dtype and np.array_equal(R.bits(g), R.bits(want)), what


def _assert_split(split, ref, n_classes, what=""):
    """ModelSplit (CUDA) against model_inputs_ref's result: upstream's shapes and dtypes, values bit for bit."""
    assert list(split.models) == list(ref["models"]), (what, list(split.models), list(ref["models"]))
    n_all = len(ref["index"])
    _same(split.abs_xyz, ref["abs_xyz"], (what, "abs_xyz"), torch.float32, (1, n_all, 3))
    _same(split.scales, ref["scales"], (what, "scales"), torch.float32, (1, n_all, 3))
    _same(split.index, ref["index"], (what, "index"), torch.int64, (n_all,))
    for name, w in ref["models"].items():
        g, n = split.models[name], len(w["index"])
        for key, dt, shape in (("abs_xyz", torch.float32, (1, n, 3)), ("rel_xyz", torch.float32, (1, n, 3)),
                               ("batch_idx", torch.int32, (1, n)), ("onehots", torch.float32, (1, n, n_classes)),
                               ("proj_uv", torch.float32, (1, n, 2)), ("classes", torch.float32, (1, n, 1)),
                               ("scales", torch.float32, (1, n, 3)), ("index", torch.int64, (n,))):
            _same(getattr(g, key), w[key], (what, name, key), dt, shape)
        assert g.abs_xyz._base is not None and g.rel_xyz.data_ptr() == g.abs_xyz.data_ptr() + 20      # views of one row
        assert split.counts[name][0] == n and split.counts[name][1] == len(np.unique(w["pts"][:, 4]))
        assert (g.zs is None) == (w["zs"] is None), (what, name)
        if w["zs"] is None:
            assert split.counts[name][2] == 0
            continue
        G = len(w["zs"])
        assert isinstance(g.zs, MI.GroupedCodes) and len(g.zs) == G == split.counts[name][2]
        _same(g.zs.group, w["group"], (what, name, "group"), torch.int32, (n,))
        _same(g.zs.codes, w["codes"], (what, name, "codes"), torch.float32, w["codes"].shape)
        _same(g.zs.instances, w["group_instances"], (what, name, "instances"), torch.int16, (G,))
        assert list(g.zs) == list(w["zs"])
        for e, v in zip(g.zs.values(), w["zs"].values()):                      # the dict it stands for, entry by entry
            _same(e["z"], v["z"], (what, name, "z"), torch.float32, v["z"].shape)
            _same(e["idx"], v["idx"], (what, name, "idx"), torch.bool, (1, n))
    for name in MI.MODELS:
        if name not in ref["models"]:
            assert split.counts[name][0] == 0


def _ref(f, table, lut, tlp=None, proj_size=2048, n_classes=8):
    return R.model_inputs_ref(f["pts"], f["batch_idx"], f["classes"], f["scales"], table, n_classes, lut, tlp, proj_size)


def _rule(table, n_classes=8):
    return MI.ModelRule(n_classes, tuple(int(v) for v in table[:n_classes]))


# ---- the recorded reference cases, through Python ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ge_all", "ge_tlp", "ge_no_bldg", "ki_all", "ki_no_car", "ki_no_rest"])
def test_golden_cases_split_and_points14(cuda_device, case):
    c = R.golden_cases(GOLDEN)[case]
    a = R.golden_inputs(c)
    ref = R.model_inputs_ref(**a)
    f = dict(pts=a["pts"], batch_idx=a["batch_idx"], instances=c["instances"], classes=a["classes"], scales=a["scales"])
    present = [bool(v) for v in c["present"]]
    make = MI.MODEL_RULE_GOOGLE_EARTH if str(c["dataset"]) == "GOOGLE_EARTH" else MI.MODEL_RULE_KITTI_360
    rule = make(present[0], rest=present[2]) if str(c["dataset"]) == "GOOGLE_EARTH" else make(*present)
    MI.reset_stats()
    split = MI.split_by_model(_visible_set(cuda_device, f), rule, _torch_lut(a["lut"]), a["tlp"], a["proj_size"])
    _assert_split(split, ref, 8, case)
    for name in ref["models"]:                          # ... and against the recorded arguments themselves
        _same(split.models[name].proj_uv, c[name + "/proj_uv"], (case, name), torch.float32, c[name + "/proj_uv"].shape)
        _same(split.models[name].batch_idx, c[name + "/batch_idx"], (case, name), torch.int32, c[name + "/batch_idx"].shape)
    attrs = {name: {str(k): torch.from_numpy(c["%s/attr_%s" % (name, k)]).to(cuda_device) for k in c["keys"]} for name in ref["models"]}
    out = MI.gaussian_points14(split, attrs)
    _same(out, c["gs_pts"], (case, "gs_pts"), torch.float32, c["gs_pts"].shape)
    assert MI.stats() == {"split_calls": 1, "points14_calls": 1}
    _same(split.abs_xyz, c["abs_xyz"], (case, "abs_xyz is not shifted in place"), torch.float32, c["abs_xyz"].shape)


# ---- random frames at the sizes where the kernels can go wrong ------------------------------------------------------------
@pytest.fixture(scope="module")
def big_case():
    """17 blocks of rows, not a multiple of 64; 2100 instances: 66 presence words per model, more than one per lane of a
    wave; three models; codes for a third of the instances, none for the first and last."""
    rng = np.random.default_rng(1701)
    ids = np.concatenate([[0, 1, 4, 5, 6], rng.choice(np.arange(100, 10000), 1535, replace=False),
                          rng.choice(np.arange(10000, 16384), 560, replace=False)])
    f = _frame(rng, 16 * BLOCK + 37, ids, first=int(ids.max()), last=int(ids.min()))
    with_code = np.setdiff1d(rng.choice(np.arange(0, 16384), 5000, replace=False), [ids.min(), ids.max(), 5])
    lut = _lut(rng, np.union1d(with_code, [4]))
    return f, lut, _ref(f, KITTI, lut, (37, -5), 1000)


def test_big_case_every_output(cuda_device, big_case):
    f, lut, ref = big_case
    assert len(f["instances"]) == 2100 and len(ref["models"]) == 3 and len(f["pts"]) % 64 and len(f["pts"]) > 3 * BLOCK
    first, last = ref["index"][0], ref["index"][-1]
    assert f["classes"][0] == 3 and f["classes"][-1] not in (2, 3, 7)          # row 0 and row M-1 in different models
    assert first != 0 and last == len(f["pts"]) - 1
    for w in ref["models"].values():
        assert (w["group"] == -1).any() and (w["group"] >= 0).any() and 0 < len(w["zs"]) < len(np.unique(w["pts"][:, 4]))
    split = MI.split_by_model(_visible_set(cuda_device, f), _rule(KITTI), _torch_lut(lut), (37, -5), 1000)
    _assert_split(split, ref, 8)


_EDGE = ["m0", "m1", "m63", "m64", "m65", "k1", "one_model", "no_car_rows", "dropped_rest", "dropped_all", "no_codes",
         "n_classes_32"]


@pytest.mark.parametrize("case", _EDGE)
def test_edge_frames(cuda_device, case):
    rng = np.random.default_rng(_EDGE.index(case) + 10)
    ids, table, n_classes, tlp, size = [1, 4, 100, 101, 340, 9999, 10000, 10020], KITTI, 8, None, 2048
    m = int(case[1:]) if case[0] == "m" else 3 * BLOCK + 5
    if case == "k1":
        ids = [101]
    elif case == "one_model":
        ids = [100, 101, 5000, 5001, 7776]                    # every row a building
    elif case == "no_car_rows":
        ids, tlp = [1, 4, 6, 100, 101], np.array([3, 9], np.int32)
    elif case == "dropped_rest":
        table, size = R.model_of_class(R.CLASS_IDS["KITTI_360"], 8, True, True, False), 1280
    elif case == "dropped_all":
        table = np.full(32, -1, np.int8)
    elif case == "n_classes_32":
        n_classes, ids = 32, list(range(0, 32)) + [100, 101]
        table = np.array([(c % 4) - 1 for c in range(32)], np.int8)
    f = _frame(rng, m, ids)
    lut = {} if case == "no_codes" else _lut(rng, ids[(0 if case == "k1" else 1)::2] + [77])
    ref = _ref(f, table, lut, tlp, size, n_classes)
    want_models = {"m0": 0, "one_model": 1, "k1": 1, "no_car_rows": 2, "dropped_rest": 2, "dropped_all": 0}.get(case)
    assert want_models is None or len(ref["models"]) == want_models, (case, list(ref["models"]))
    if case == "no_codes":
        assert all(w["zs"] is None for w in ref["models"].values())
    split = MI.split_by_model(_visible_set(cuda_device, f), _rule(table, n_classes), _torch_lut(lut) if lut else None, tlp, size)
    _assert_split(split, ref, n_classes, case)
    attrs = {name: {"rgb": torch.rand((1, len(w["index"]), 3), device=cuda_device)} for name, w in ref["models"].items()}
    out = MI.gaussian_points14(split, attrs)                   # (an empty split gives an empty tensor)
    assert tuple(out.shape) == (1, len(ref["index"]), 14)


# ---- the C ABI by hand: poison, canaries, NULL outputs, stale workspaces --------------------------------------------------
_OUT = (("index", torch.int64, 1), ("pts", torch.float32, 8), ("batch", torch.int32, 1), ("classes", torch.float32, 1),
        ("scales", torch.float32, 3), ("onehots", torch.float32, 8), ("proj_uv", torch.float32, 2), ("group", torch.int32, 1),
        ("group_instances", torch.int16, 1), ("codes", torch.float32, 12))


class _Raw:
    def __init__(self, dev, f, lut, table=KITTI, tlp=(0, 0), size=2048, ws=None):
        self.L, self.dev = V.lib(), dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.f = {k: t(v) for k, v in f.items()}
        self.m, self.k = len(f["pts"]), len(f["instances"])
        st = MI.StyleTable(_torch_lut(lut), dev)
        self.st, self.rule = st, MI._native_rule(_rule(table), np.array(tlp, np.int32), size)
        self.nb = self.L.gcv_model_split_workspace_bytes(self.m, self.k)
        # the workspace between two canary regions, filled with stale garbage
        self.ws_all = ws if ws is not None else torch.randint(0, 256, (self.nb + 512,), dtype=torch.uint8, device=dev)
        self.ws_all[:256], self.ws_all[256 + self.nb:] = 0xA5, 0xA5
        self.ws = self.ws_all[256:256 + self.nb]

    def ws_canaries_intact(self):
        return bool((self.ws_all[:256] == 0xA5).all()) and bool((self.ws_all[256 + self.nb:] == 0xA5).all())

    def count(self):
        counts = (C.c_int64 * 9)(*[-9] * 9)
        f = self.f
        rc = self.L.gcv_model_split_count(f["classes"].data_ptr(), f["batch_idx"].data_ptr(), self.m, f["instances"].data_ptr(),
                                          self.k, self.st.lut_has.data_ptr(), self.st.n_lut, C.byref(self.rule),
                                          self.ws.data_ptr(), self.nb, counts, None)
        return rc, list(counts)

    def outputs(self, n, g):
        """Every output between two canary regions, the payload poisoned (NaN bit patterns / -1)."""
        o = {}
        for name, dt, width in _OUT:
            rows = g if name in ("group_instances", "codes") else n
            buf = torch.full(((rows + 2 * CANARY) * width,), float("nan") if dt == torch.float32 else -1, dtype=dt, device=self.dev)
            o[name] = buf
        return o

    @staticmethod
    def payload(o, name, rows):
        width = dict((n, w) for n, _, w in _OUT)[name]
        return o[name][CANARY * width:(CANARY + rows) * width]

    @staticmethod
    def canaries_intact(o, name, rows):
        width = dict((n, w) for n, _, w in _OUT)[name]
        edge = torch.cat([o[name][:CANARY * width], o[name][(CANARY + rows) * width:]])
        return bool((torch.isnan(edge) if edge.dtype == torch.float32 else edge == -1).all())

    def emit(self, counts, o, skip=()):
        f, width = self.f, dict((n, w) for n, _, w in _OUT)
        ptr = lambda name: None if name in skip else o[name].data_ptr() + CANARY * width[name] * o[name].element_size()  # noqa: E731
        rc = self.L.gcv_model_split_emit(
            f["classes"].data_ptr(), f["batch_idx"].data_ptr(), f["pts"].data_ptr(), f["scales"].data_ptr(), self.m,
            f["instances"].data_ptr(), self.k, self.st.lut_has.data_ptr(), self.st.lut.data_ptr(), self.st.n_lut, self.st.z_dim,
            C.byref(self.rule), self.ws.data_ptr(), self.nb, (C.c_int64 * 9)(*counts), *[ptr(name) for name, _, _ in _OUT], None)
        torch.cuda.synchronize()
        return rc


def _raw_want(ref):
    """model_inputs_ref's per-model arrays concatenated as the C ABI lays them out."""
    ms = list(ref["models"].values())
    cat = lambda key: np.concatenate([w[key] for w in ms])   # noqa: E731
    with_z = [w for w in ms if w["zs"] is not None]
    return {"index": cat("index"), "pts": cat("pts"), "batch": cat("batch_idx"), "classes": cat("classes"), "scales": cat("scales"),
            "onehots": cat("onehots"), "proj_uv": cat("proj_uv"),
            "group": np.concatenate([w["group"] if w["zs"] is not None else np.full(len(w["index"]), -1, np.int32) for w in ms]),
            "group_instances": np.concatenate([w["group_instances"] for w in with_z]),
            "codes": np.concatenate([w["codes"] for w in with_z])}


@pytest.fixture(scope="module")
def raw_case():
    rng = np.random.default_rng(1702)
    ids = [1, 4, 5, 6, 100, 101, 340, 341, 2000, 2001, 2002, 9999, 10000, 10003, 10010, 12000]
    f = _frame(rng, 3 * BLOCK + 77, ids)
    lut = _lut(rng, [4, 101, 341, 2001, 10003, 12000, 555])
    return f, lut, _ref(f, KITTI, lut, (11, 2), 1280)


def test_raw_poison_canaries_and_null_outputs(cuda_device, raw_case):
    f, lut, ref = raw_case
    raw = _Raw(cuda_device, f, lut, tlp=(11, 2), size=1280)
    rc, counts = raw.count()
    ms = ref["models"]
    assert rc == 0 and counts[:3] == [len(ms[k]["index"]) for k in R.MODELS]
    assert counts[3:6] == [len(np.unique(ms[k]["pts"][:, 4])) for k in R.MODELS] and counts[6:] == [len(ms[k]["zs"]) for k in R.MODELS]
    n, g = sum(counts[:3]), sum(counts[6:])
    want = _raw_want(ref)
    o = raw.outputs(n, g)
    assert raw.emit(counts, o) == 0 and raw.ws_canaries_intact()
    for name, dt, width in _OUT:
        rows = g if name in ("group_instances", "codes") else n
        assert raw.canaries_intact(o, name, rows), name
        got = raw.payload(o, name, rows).cpu().numpy().reshape(want[name].shape)
        assert np.array_equal(R.bits(got), R.bits(want[name])), name       # every element written: no poison is a wanted value
    for skip in (("index",), ("pts", "proj_uv"), ("group", "group_instances", "codes"), ("batch", "classes", "scales", "onehots"),
                 tuple(name for name, _, _ in _OUT if name != "codes")):
        o2 = raw.outputs(n, g)
        assert raw.emit(counts, o2, skip=skip) == 0
        for name, _, _ in _OUT:
            if name in skip:
                p = o2[name]
                assert bool((torch.isnan(p) if p.dtype == torch.float32 else p == -1).all()), (skip, name)
            else:
                assert torch.equal(o2[name].view(torch.uint8), o[name].view(torch.uint8)), (skip, name)


def test_one_workspace_two_frames_and_stale_garbage(cuda_device, raw_case, big_case):
    """The larger frame, then a smaller one, then the larger again through one garbage-filled workspace: every count clears
    what it uses, so nothing of the frame before survives."""
    (fa, la, ra), (fb, lb, rb) = big_case[:3], raw_case
    ws = P.VisibleSetWorkspace(cuda_device)
    need = V.lib().gcv_model_split_workspace_bytes(len(fa["pts"]), len(fa["instances"]))
    ws.take(need).copy_(torch.randint(0, 256, (need,), dtype=torch.uint8, device=cuda_device))
    buf = ws.buf
    sets = [(_visible_set(cuda_device, f), _torch_lut(lut)) for f, lut in ((fa, la), (fb, lb))]
    got = [MI.split_by_model(sets[0][0], _rule(KITTI), sets[0][1], (37, -5), 1000, workspace=ws),
           MI.split_by_model(sets[1][0], _rule(KITTI), sets[1][1], (11, 2), 1280, workspace=ws),
           MI.split_by_model(sets[0][0], _rule(KITTI), sets[0][1], (37, -5), 1000, workspace=ws)]
    for s, r, name in zip(got, (ra, rb, ra), "aba"):
        _assert_split(s, r, 8, name)
    assert ws.buf is buf


@pytest.mark.parametrize("bad", ["class_8", "class_minus_1", "class_2_5", "class_nan", "class_huge", "rank_minus_1", "rank_k", "rank_huge"])
def test_bad_class_or_rank_is_refused_and_indexes_nothing(cuda_device, raw_case, bad):
    f, lut, _ = raw_case
    f = {k: v.copy() for k, v in f.items()}
    rows = [0, 300, len(f["pts"]) - 1]
    if bad.startswith("class"):
        f["classes"][rows] = {"class_8": 8.0, "class_minus_1": -1.0, "class_2_5": 2.5, "class_nan": np.nan, "class_huge": 3e38}[bad]
    else:
        f["batch_idx"][rows] = {"rank_minus_1": -1, "rank_k": len(f["instances"]), "rank_huge": 2 ** 31 - 1}[bad]
    raw = _Raw(cuda_device, f, lut)
    rc, counts = raw.count()
    assert rc == INVALID and b"3 row(s)" in raw.L.gcv_last_error() and counts == [-9] * 9 and raw.ws_canaries_intact()
    with pytest.raises(RuntimeError, match="gcv_status -1"):
        MI.split_by_model(_visible_set(cuda_device, f), _rule(KITTI), _torch_lut(lut))
    # an emit all the same, with the counts of the good rows: the bad rows are dropped, nothing lands outside the outputs
    good = {k: np.delete(v, rows, axis=0) if k != "instances" else v for k, v in f.items()}
    ref = R.model_inputs_ref(good["pts"], good["batch_idx"], good["classes"], good["scales"], KITTI, 8, lut, (0, 0), 2048)
    want = _raw_want(ref)
    ms = ref["models"]
    counts = [len(ms[k]["index"]) for k in R.MODELS] + [len(np.unique(ms[k]["pts"][:, 4])) for k in R.MODELS] + \
             [len(ms[k]["zs"]) for k in R.MODELS]
    n, g = sum(counts[:3]), sum(counts[6:])
    o = raw.outputs(n, g)
    assert raw.emit(counts, o) == 0 and raw.ws_canaries_intact()
    for name, _, _ in _OUT:
        assert raw.canaries_intact(o, name, g if name in ("group_instances", "codes") else n), name
    for name in ("pts", "batch", "classes", "scales", "onehots", "proj_uv", "group"):         # the good rows, in order
        got = raw.payload(o, name, n).cpu().numpy().reshape(want[name].shape)
        assert np.array_equal(R.bits(got), R.bits(want[name])), name


# ---- [N,14] ------------------------------------------------------------------------------------------------------------
def test_points14_every_key_subset_one_two_three_segments(cuda_device, raw_case):
    f, lut, ref = raw_case
    vs = _visible_set(cuda_device, f)
    gen = torch.Generator(device=cuda_device).manual_seed(3)
    width = {"rgb": 3, "xyz": 3, "scale": 3, "opacity": 1}
    tables = {3: KITTI, 2: R.model_of_class(R.CLASS_IDS["KITTI_360"], 8, True, False, True),
              1: R.model_of_class(R.CLASS_IDS["KITTI_360"], 8, False, False, True)}
    for segments, table in tables.items():
        split = MI.split_by_model(vs, _rule(table))
        assert len(split.models) == segments and split.pts.shape[1] > 3 * BLOCK
        for r in range(4):
            for extra in itertools.combinations(("xyz", "scale", "opacity"), r):
                keys = ("rgb",) + extra
                attrs = {name: {k: torch.rand((1, m.index.shape[0], width[k]), generator=gen, device=cuda_device) * 2 - 0.5
                                for k in keys} for name, m in split.models.items()}
                got = MI.gaussian_points14(split, attrs)
                cat = {k: torch.cat([a[k] for a in attrs.values()], dim=1) for k in keys}
                want = H.get_gaussian_points(split.abs_xyz.clone(), split.scales.clone(), cat)
                assert got.dtype == want.dtype and got.shape == want.shape == (1, split.pts.shape[1], 14)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (segments, keys)
                got2 = MI.gaussian_points14(split, list(attrs.values()))           # a sequence in the models' order
                assert torch.equal(got2.view(torch.int32), got.view(torch.int32))
    # dicts that disagree, a missing rgb, a wrong shape
    names = list(split.models)
    n0 = split.models[names[0]].index.shape[0]
    rgb = torch.rand((1, n0, 3), device=cuda_device)
    split3 = MI.split_by_model(vs, _rule(KITTI))
    a3 = {name: {"rgb": torch.rand((1, m.index.shape[0], 3), device=cuda_device)} for name, m in split3.models.items()}
    a3["CAR"]["opacity"] = torch.rand((1, split3.models["CAR"].index.shape[0], 1), device=cuda_device)
    with pytest.raises(ValueError, match="same keys"):
        MI.gaussian_points14(split3, a3)
    with pytest.raises(ValueError, match="rgb"):
        MI.gaussian_points14(split, {names[0]: {"xyz": rgb}})
    with pytest.raises(ValueError):
        MI.gaussian_points14(split3, {names[0]: {"rgb": rgb}})
    with pytest.raises(TypeError):
        MI.gaussian_points14(split, {names[0]: {"rgb": rgb[:, :-1]}})
