"""-m gpu: gaussiancity_amd.train_inputs (include/gcv.h K23 / K24) against the restatement of core/train.py:207-224
(tests/train_inputs_ref.py) and the reference's recorded results (tests/golden/train_inputs.npz).  Every comparison is bit
for bit on all rows: every value is an integer or one rounded float32 operation.  The style codes are compared with the
draws of the default CPU generator from the same seed, and so is the generator's state afterwards."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import operand_views as OV
import train_inputs_ref as R
from test_train_inputs_host import CASES, GOLDEN, golden_case

pytestmark = pytest.mark.gpu
SEED = 77
FIELDS = ("bch_idx", "classes", "scales", "onehots", "proj_uv")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_v
    _native_v.lib()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def T():
    from gaussiancity_amd import train_inputs
    return train_inputs


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def make_pts(ids, n, seed, b=1):
    """[b, n, 9] rows as the loader makes them: every id at least once where n allows, in no order; coordinates and scales
    that are no integers, so the float32 operations round."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.tensor(sorted(ids), dtype=torch.float32)
    pts = torch.empty(b, n, 9)
    pts[:, :, :3] = torch.rand(b, n, 3, generator=gen) * 2048
    pts[:, :, 3] = torch.rand(b, n, generator=gen) * 4 + 0.5
    for k in range(b):
        ins = ids[torch.randint(0, len(ids), (n,), generator=gen)]
        m = min(n, len(ids))
        ins[torch.randperm(n, generator=gen)[:m]] = ids[torch.randperm(len(ids), generator=gen)[:m]]
        pts[k, :, 4] = ins
        pts[k, :, 8] = torch.searchsorted(torch.unique(ins), ins).float()
    pts[:, :, 5:8] = torch.rand(b, n, 3, generator=gen) * 2 - 1
    return pts


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def check(T, dev, pts, rule, z_dim=None, tlp=None, pts_dev=None, **kw):
    """prepare on the device against the restatement, all rows; with a z_dim also the groups, the ids, the codes as I
    draws from the same seed, and the generator's state afterwards.  Returns the TrainInputs."""
    want = R.restate(pts, rule, None, None if tlp is None else torch.as_tensor(tlp).cpu())
    if z_dim is not None:
        group, ids = R.groups(pts, rule)
        torch.manual_seed(SEED)
        codes = torch.cat([torch.randn(1, z_dim) for _ in ids] + [torch.empty(0, z_dim)])
        state = torch.get_rng_state()
    torch.manual_seed(SEED)
    src = pts.to(dev) if pts_dev is None else pts_dev
    got = T.prepare(src, rule, z_dim, tlp, **kw)
    for k in FIELDS:
        assert bits(getattr(got, k), want[k]), k
    assert got.abs_xyz.data_ptr() == src.data_ptr() and bits(got.abs_xyz, pts[:, :, :3])
    assert bits(got.rel_xyz, pts[:, :, 5:8]) and bits(got.instances, pts[:, :, 4:5])
    assert got.flag.dtype == torch.int32 and got.flag.dim() == 0 and got.flag.is_cuda and int(got.flag) == want["flagged"]
    if z_dim is None:
        assert got.z is None
        return got
    z = got.z
    assert z.group.dtype == torch.int32 and z.instances.dtype == torch.int16 and z.codes.dtype == torch.float32
    assert bits(z.group, group) and bits(z.instances, ids) and bits(z.codes, codes)
    assert torch.equal(torch.get_rng_state(), state)
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 16384])
def test_row_counts(T, dev, n):
    pts = make_pts([1, 3, 5, 6, 100, 101, 230, 4444, 32767], n, n)
    check(T, dev, pts, T.RULE_GOOGLE_EARTH(), 8, torch.tensor([[37, 1205]]))
    check(T, dev, pts, T.RULE_GOOGLE_EARTH(), None, None)


SEAMS = {"zero": [0], "31_32": [31, 32], "63_64": [63, 64], "1023_1024": [1023, 1024], "32767": [32767], "single": [230],
         "256": list(range(100, 32768, 128))[:255] + [32767]}


@pytest.mark.parametrize("name", list(SEAMS))
def test_instance_ids_on_the_tables_seams(T, dev, name):
    ids = SEAMS[name]
    rule = T.RULE_GOOGLE_EARTH()._replace(bldg_ins_min=8)        # every id from 8 on is a building: its class is in the one-hot
    got = check(T, dev, make_pts(ids, 300, len(ids)), rule, 8)
    assert len(got.z) == len(ids) == len(set(ids)) and list(got.z) == sorted(ids)


def test_building_ids_at_both_ends_of_the_range_in_both_parities(T, dev):
    rule = T.RULE_GOOGLE_EARTH()
    ids = [6, rule.bldg_ins_min, rule.bldg_ins_min + 1, rule.bldg_ins_max - 2, rule.bldg_ins_max - 1]
    pts = make_pts(ids, 65, 3)
    got = check(T, dev, pts, rule, 8)
    want = {6: 6.0, 100: 2.0, 101: 7.0, 32766: 2.0, 32767: 7.0}
    assert got.classes[0, :, 0].tolist() == [want[int(i)] for i in pts[0, :, 4]]


def test_car_range_at_both_ends_and_the_car_class_wins_an_overlap(T, dev):
    rule = T.RULE_KITTI_360()
    ids = [1, 9998, 9999, 10000, 10001, 16382, 16383]
    pts = make_pts(ids, 65, 4)
    got = check(T, dev, pts, rule, 8)
    want = {1: 1.0, 9998: 2.0, 9999: 7.0, 10000: 3.0, 10001: 3.0, 16382: 3.0, 16383: 3.0}
    assert got.classes[0, :, 0].tolist() == [want[int(i)] for i in pts[0, :, 4]]
    flagged = make_pts(ids + [16384], 65, 4)                     # one past the car range keeps its id: no class of the one-hot
    assert int(check(T, dev, flagged, rule).flag) == int((flagged[0, :, 4] == 16384).sum())
    overlap = rule._replace(car_ins_min=5000)                     # 5000..9999 lie in both ranges
    pts = make_pts([4999, 5000, 5001, 9999, 10000], 65, 5)
    got = check(T, dev, pts, overlap, 8)
    want = {4999: 7.0, 5000: 3.0, 5001: 3.0, 9999: 3.0, 10000: 3.0}
    assert got.classes[0, :, 0].tolist() == [want[int(i)] for i in pts[0, :, 4]]


@pytest.mark.parametrize("dataset", ["GOOGLE_EARTH", "KITTI_360"])
def test_each_special_z_class(T, dev, dataset):
    rule = getattr(T, "RULE_" + dataset)()
    pts = make_pts(list(range(8)) + [100, 101], 257, 6)
    got = check(T, dev, pts, rule)
    special = torch.isin(pts[0, :, 4], torch.tensor(rule.special_z_classes, dtype=torch.float32))
    assert special.sum() >= len(rule.special_z_classes)
    z = got.scales[0, :, 2].cpu()
    assert bool((z[special] == 1).all()) and bool((z[~special] == got.scales[0, :, 0].cpu()[~special]).all())


def test_one_hot_widths_of_1_and_32(T, dev):
    one = T.RULE_GOOGLE_EARTH()._replace(n_classes=1, facade_class=0, roof_class=0, special_z_classes=(0,))
    got = check(T, dev, make_pts([0, 100, 101, 32767], 65, 7), one, 8)
    assert got.onehots.shape == (1, 65, 1) and bool((got.onehots == 1).all())
    wide = T.RULE_KITTI_360()._replace(n_classes=32, car_class=31, special_z_classes=(1, 31))
    got = check(T, dev, make_pts(list(range(32)) + [100, 101, 10000], 257, 8), wide, 8)
    assert got.onehots.shape == (1, 257, 32) and bool((got.onehots.sum(-1) == 1).all())
    odd = T.RULE_KITTI_360()._replace(n_classes=9)                # a width that is no multiple of 4: the scalar stores
    check(T, dev, make_pts(list(range(9)) + [100, 101, 10000], 257, 9), odd)


def test_two_crops_with_a_top_left_point_each(T, dev):
    pts = make_pts([1, 5, 6, 100, 101, 9999, 10000], 65, 10, b=2)
    rule = T.RULE_KITTI_360()
    tlp = torch.tensor([[37, 1205], [-12, 640]])
    check(T, dev, pts, rule, None, tlp.to(dev))                                   # int64 on the device
    check(T, dev, pts, rule, None, tlp.float().to(dev))                           # float32 on the device
    check(T, dev, pts, rule, None, tlp.numpy())                                   # a host array
    check(T, dev, pts, rule, None, None)
    with pytest.raises(AssertionError, match=r"Unexpected tensor shape \(2, 65, 1\)"):
        T.prepare(pts.to(dev), rule, 8)
    with pytest.raises(TypeError, match="float64"):
        T.prepare(pts.to(dev), rule, None, tlp.double())
    with pytest.raises(ValueError, match="two values"):
        T.prepare(pts.to(dev), rule, None, tlp[:1])


@pytest.mark.parametrize("value", [2.5, -1.0, float("nan"), 32768.0, 9.0])
def test_flagged_rows(T, dev, value):
    """2.5, -1, NaN and 32768 are no instance ids; 9 is one, and a class it keeps that the 8-wide one-hot does not have."""
    rule = T.RULE_KITTI_360()
    pts = make_pts([1, 5, 100, 101, 10000], 257, 11)
    clean = check(T, dev, pts, rule, 8)
    dirty = pts.clone()
    dirty[0, 200, 4] = value
    got = check(T, dev, dirty, rule, 8)
    assert int(got.flag) == 1
    assert bool((got.onehots[0, 200] == 0).all()) and int(got.z.group[200]) == -1
    keep = torch.arange(257) != 200
    for k in FIELDS:
        assert bits(getattr(got, k)[:, keep], getattr(clean, k)[:, keep]), k
    if value != 9.0:                                              # (9 is an id, and has its place among the groups)
        assert bits(got.z.group[keep], clean.z.group[keep]) and bits(got.z.instances, clean.z.instances)
    else:
        assert got.z.instances.tolist() == [1, 5, 9, 100, 101, 10000]
    assert int(check(T, dev, dirty, rule).flag) == 1              # and without a count in front
    for z_dim in (None, 8):
        with pytest.raises(ValueError, match="1 row"):
            T.prepare(dirty.to(dev), rule, z_dim, check=True)
    assert int(T.prepare(pts.to(dev), rule, None, check=True).flag) == 0     # the flag does not stick


def test_the_count_reports_distinct_instances_and_flagged_ids(T, dev):
    from gaussiancity_amd import _native_v as V
    from gaussiancity_amd._loader import current_stream
    pts = make_pts([1, 5, 100, 101, 10000], 257, 12)
    pts[0, 3, 4], pts[0, 250, 4], pts[0, 100, 4] = 2.5, float("nan"), 9.0
    d = pts.to(dev)
    ws = T.Workspace(dev)
    counts = (C.c_int64 * 2)()
    V.check(V.lib().gcv_train_inputs_count(d.data_ptr(), 9, 257, ws.buf.data_ptr(), ws.buf.numel(), counts, current_stream()), "count")
    assert list(counts) == [6, 2]                                 # 9 is an id; its class is the emit's to flag
    assert int(check(T, dev, pts, T.RULE_KITTI_360(), 8, workspace=ws).flag) == 3


def test_one_workspace_serves_disjoint_sets_without_stale_bits(T, dev):
    ws, rule = T.Workspace(dev), T.RULE_GOOGLE_EARTH()
    a = check(T, dev, make_pts([1, 100, 101, 1023, 32767], 257, 13), rule, 8, workspace=ws)
    b = check(T, dev, make_pts([3, 5, 230, 1024, 32766], 65, 14), rule, 8, workspace=ws)
    assert list(a.z) == [1, 100, 101, 1023, 32767] and list(b.z) == [3, 5, 230, 1024, 32766]
    check(T, dev, make_pts([6], 64, 15), rule, None, workspace=ws)
    assert b.flag.data_ptr() == ws.flag.data_ptr()


def test_two_runs_give_equal_bits(T, dev):
    pts = make_pts(list(range(100, 32768, 331)), 16384, 16).to(dev)
    rule = T.RULE_GOOGLE_EARTH()
    runs = []
    for _ in range(2):
        torch.manual_seed(SEED)
        runs.append(T.prepare(pts, rule, 8, torch.tensor([[5, 9]])))
    for k in FIELDS:
        assert bits(getattr(runs[0], k), getattr(runs[1], k)), k
    assert all(bits(getattr(runs[0].z, k), getattr(runs[1].z, k)) for k in ("group", "codes", "instances"))


@pytest.mark.parametrize("kind", ["offset", "ragged_rows", "expanded"])
@pytest.mark.parametrize("b", [1, 2])
def test_strided_views_give_the_dense_calls_bits(T, dev, kind, b):
    pts = make_pts([1, 5, 100, 101, 9999, 10000], 257, 17, b=b)
    built = OV.build(kind, pts.to(dev), 1)                        # (expanded: along the rows, every row the first)
    twin = built.view.contiguous().cpu()
    z_dim, tlp = (8, None) if b == 1 else (None, torch.tensor([[3, 4], [5, 6]]))
    before = built.base.clone()
    got = check(T, dev, twin, T.RULE_KITTI_360(), z_dim, tlp, pts_dev=built.view)
    assert bits(built.base, before)                               # pts is read only, filler included
    assert got.instances.data_ptr() == built.view[:, :, 4:5].data_ptr()


@pytest.mark.parametrize("name", CASES)
def test_the_recorded_cases(T, dev, golden, name):
    """What the reference's own lines computed: the dict of get_z through GroupedCodes' mapping interface, the codes and
    the generator's end state included."""
    pts, rule, z_dim, tlp = golden_case(golden, name)
    torch.set_rng_state(torch.from_numpy(golden["rng_before"]))
    got = T.prepare(pts.to(dev), rule, z_dim, tlp)
    for k in FIELDS:
        assert bits(getattr(got, k), torch.from_numpy(golden[name + "/" + k])), k
    assert int(got.flag) == 0
    if z_dim is None:
        assert got.z is None and torch.equal(torch.get_rng_state(), torch.from_numpy(golden["rng_before"]))
        return
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(golden[name + "/rng_after"]))
    z = got.z
    assert list(z.keys()) == golden[name + "/z_keys"].tolist() == list(z)
    entries = z.values()
    assert all(sorted(e) == ["idx", "z"] and e["z"].shape == (1, z_dim) and e["idx"].shape == (1, 300) for e in entries)
    assert bits(torch.cat([e["z"] for e in entries]), torch.from_numpy(golden[name + "/z_codes"]))
    assert np.array_equal(np.packbits(torch.cat([e["idx"] for e in entries]).cpu().numpy(), axis=1), golden[name + "/z_idx"])
    assert torch.equal(got.bch_idx[0], z.group.long())            # NormalizePointCords numbers the instances the same way


def test_get_z_is_a_drop_in(T, dev, golden):
    pts, rule, z_dim, _ = golden_case(golden, "ki/z8")
    instances = pts[:, :, [4]].to(dev)
    T.reset_stats()
    torch.set_rng_state(torch.from_numpy(golden["rng_before"]))
    z = T.get_z(instances, z_dim)
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(golden["ki/z8/rng_after"]))
    assert list(z) == golden["ki/z8/z_keys"].tolist()
    assert bits(z.codes, torch.from_numpy(golden["ki/z8/z_codes"]))
    assert np.array_equal(np.packbits(torch.cat([e["idx"] for e in z.values()]).cpu().numpy(), axis=1), golden["ki/z8/z_idx"])
    assert T.get_z(instances, None) is None
    with pytest.raises(AssertionError, match=r"Unexpected tensor shape \(2, 150, 1\)"):
        T.get_z(instances.reshape(2, 150, 1), z_dim)
    helpers = types.SimpleNamespace(get_z=lambda instances, z_dim: "original")
    T.install(helpers)
    try:
        torch.set_rng_state(torch.from_numpy(golden["rng_before"]))
        installed = helpers.get_z(instances, z_dim)
        assert bits(installed.codes, z.codes) and bits(installed.group, z.group)
        assert helpers.get_z(instances.cpu(), z_dim) == "original"
    finally:
        T.uninstall(helpers)
    assert T.stats() == {"prepare_calls": 0, "get_z_calls": 2}


def test_stats_count_the_calls(T, dev):
    T.reset_stats()
    pts = make_pts([1, 100], 64, 18).to(dev)
    T.prepare(pts, T.RULE_GOOGLE_EARTH())
    T.prepare(pts, T.RULE_GOOGLE_EARTH(), 8)
    assert T.stats() == {"prepare_calls": 2, "get_z_calls": 0}
    T.reset_stats()
    assert T.stats() == {"prepare_calls": 0, "get_z_calls": 0}


def test_no_rows(T, dev):
    got = T.prepare(torch.empty(1, 0, 9, device=dev), T.RULE_GOOGLE_EARTH(), 8)
    assert got.bch_idx.shape == (1, 0) and got.bch_idx.dtype == torch.int64 and got.onehots.shape == (1, 0, 8)
    assert got.classes.shape == (1, 0, 1) and got.scales.shape == (1, 0, 3) and got.proj_uv.shape == (1, 0, 2)
    assert len(got.z) == 0 and got.z.codes.shape == (0, 8) and int(got.flag) == 0
    assert T.prepare(torch.empty(2, 0, 9, device=dev), T.RULE_GOOGLE_EARTH()).z is None


def test_the_attribute_head_takes_z_without_folding_masks(T, dev):
    from gaussiancity_amd import _native_m, attr_head, modlinear
    from test_model_inputs_attr_gpu import IN_DIM, Z_DIM, _stand_in
    _native_m.lib()
    pts = make_pts([1, 4, 100, 101, 340, 341, 2000, 10000], 600, 19)
    torch.manual_seed(SEED)
    got = T.prepare(pts.to(dev), T.RULE_KITTI_360(), Z_DIM)
    assert attr_head.grouped_ok(got.z, 600)
    as_dict = {i: {"z": v["z"].clone(), "idx": v["idx"].clone()} for i, v in got.z.items()}     # what get_z returns
    feat = torch.randn((1, 600, IN_DIM), generator=torch.Generator().manual_seed(20)).to(dev)
    torch.manual_seed(21)
    G = _stand_in()
    head = G.GaussianAttrMLP().to(dev)
    attr_head.install(G)
    try:
        with torch.no_grad():
            attr_head.reset_stats()
            modlinear.reset_stats()
            from_dict = head(feat, got.onehots, as_dict)
            assert attr_head.grouped_stats() == {"grouped_calls": 0} and modlinear.stats()["groups_from_masks_calls"] == 1
            grouped = head(feat, got.onehots, got.z)
            assert attr_head.stats() == {"fused_calls": 2, "original_calls": 0} and attr_head.grouped_stats() == {"grouped_calls": 1}
            assert modlinear.stats()["groups_from_masks_calls"] == 1                      # no masks were folded
        assert list(grouped) == list(from_dict) and all(bits(grouped[k], from_dict[k]) for k in grouped)
    finally:
        attr_head.uninstall(G)
