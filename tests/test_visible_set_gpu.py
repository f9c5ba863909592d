"""-m gpu: the visible point set on the device (gaussiancity_amd.points.visible_point_set -> gcv_visible_count /
gcv_visible_emit -> gfx950 kernels) against the numpy formulation in visible_ref.py.  Index work plus binary64
arithmetic in a fixed order rounded once to binary32, so the bar is BIT-EXACT for every output."""
import ctypes as C

import numpy as np
import pytest
import torch

from gaussiancity_amd import _native_v as V
from gaussiancity_amd import points as P
from gaussiancity_amd import synth
from visible_ref import visible_ref

pytestmark = pytest.mark.gpu

SCAN_BLOCK_POINTS = 32768   # one block of the count / emit kernels: 256 threads x 4 bitmap words x 32 points
N_RANDOM = 100_003          # > 2 * SCAN_BLOCK_POINTS (four blocks), not a multiple of 32 or 64
INVALID = -1


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want, what=""):
    """VisibleSet (CUDA) against visible_ref's dict: shapes and dtypes of render()'s tensors, values bit for bit."""
    m, k = len(want["index"]), len(want["instances"])
    shapes = {"index": (m,), "pts": (1, m, 8), "batch_idx": (1, m, 1), "instances": (k,), "classes": (1, m, 1), "scales": (1, m, 3)}
    dtypes = {"index": torch.int64, "pts": torch.float32, "batch_idx": torch.int32, "instances": torch.int16,
              "classes": torch.float32, "scales": torch.float32}
    for key in shapes:
        t = getattr(got, key)
        assert tuple(t.shape) == shapes[key] and t.dtype == dtypes[key], (what, key, tuple(t.shape), t.dtype)
        g = t.cpu().numpy().reshape(want[key].shape)
        assert np.array_equal(_bits(g), _bits(want[key])), (what, key)


def _run(dev, rows, vp_map, centers, rule, **kw):
    table = centers if isinstance(centers, dict) else torch.from_numpy(centers).to(dev)
    return P.visible_point_set(torch.from_numpy(rows).to(dev), torch.from_numpy(vp_map).to(dev), table, rule, **kw)


def _random_rows(rng, n, n_instances):
    rows = np.empty((n, 5), np.int16)
    rows[:, :3] = rng.integers(-300, 2300, (n, 3))
    rows[:, 3] = rng.integers(1, 5, n)
    rows[:, 4] = rng.integers(0, n_instances, n)
    return rows


def _random_table(rng, n_instances):
    """Boxes with non-integer centres; a few with a zero extent."""
    t = np.empty((n_instances, 5), np.float64)
    t[:, :2] = rng.uniform(0, 2048, (n_instances, 2))
    t[:, 2:] = rng.uniform(0.5, 700, (n_instances, 3))
    t[rng.integers(0, n_instances, 6), rng.integers(2, 5, 6)] = 0.0
    return t


def _random_map(rng, n, shape, pool, negative=0.3):
    ids = rng.choice(n, pool, replace=False)
    vp = ids[rng.integers(0, pool, shape)].astype(np.int64)
    vp[rng.random(shape) < negative] = -1
    return vp


@pytest.fixture(scope="module")
def random_case():
    rng = np.random.default_rng(1601)
    rows, table = _random_rows(rng, N_RANDOM, 300), _random_table(rng, 300)
    vp = _random_map(rng, N_RANDOM, (24, 40), 350)
    vp[5, 7], vp[20, 3] = -5, -(2 ** 40)    # any negative value means "no point"
    vp[0, 0], vp[0, 1] = N_RANDOM - 1, 0    # the first bit of the first block and the last bit of the last
    return rows, table, vp, visible_ref(rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH)


def test_random_case_all_six_outputs(cuda_device, random_case):
    rows, table, vp, want = random_case
    assert (vp < 0).mean() > 0.2 and len(want["index"]) < (vp >= 0).sum() and len(want["index"]) > 200
    assert want["index"].min() < SCAN_BLOCK_POINTS and want["index"].max() > 3 * SCAN_BLOCK_POINTS   # first and last block
    _assert_same(_run(cuda_device, rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH), want)


_EDGE = ["all_negative", "same_id", "first_and_last", "n1", "n31", "n32", "n33", "n64", "n65"]


@pytest.mark.parametrize("case", _EDGE)
def test_edge_maps(cuda_device, case):
    rng = np.random.default_rng(99)
    if case.startswith("n"):
        n = int(case[1:])
        vp = rng.permutation(np.repeat(np.arange(n, dtype=np.int64), 2)).reshape(2, n)   # every point visible, twice
    else:
        n = 1000 + 37    # a partial last bitmap word
        vp = {"all_negative": np.full((6, 9), -1, np.int64), "same_id": np.full((6, 9), 517, np.int64),
              "first_and_last": np.array([[n - 1, -1, 0, 500, n - 1, 0]], np.int64)}[case]
    rows, table = _random_rows(rng, n, 40), _random_table(rng, 40)
    want = visible_ref(rows, vp, table, P.CLASS_RULE_KITTI_360)
    assert len(want["index"]) == {"all_negative": 0, "same_id": 1, "first_and_last": 3}.get(case, n)
    _assert_same(_run(cuda_device, rows, vp, table, P.CLASS_RULE_KITTI_360), want, case)


def test_relative_coordinates_bit_for_bit(cuda_device):
    """The zero branches (w, h, d = 0, one at a time and all three), z / d * 2 - 1 beyond both clip ends, non-integer
    centres, extents that do not divide evenly, and coordinates at +-32767."""
    table = np.array([[10.25, -3.7, 0.0, 5.0, 7.0],           # 0: w = 0
                      [10.25, -3.7, 3.0, 0.0, 7.0],           # 1: h = 0
                      [10.25, -3.7, 3.0, 5.0, 0.0],           # 2: d = 0
                      [0.0, 0.0, 0.0, 0.0, 0.0],              # 3: all three
                      [1023.1, 1024.9, 0.3, 1e-3, 3.3],       # 4: tiny extents: large quotients; z clips at +1
                      [-32767.5, 32767.5, 65535.0, 7.0, 1e9],  # 5: huge depth: z / d * 2 - 1 just above -1
                      [1.0 / 3.0, 2.0 / 3.0, 1.0 / 7.0, 1.0 / 11.0, 1.0 / 13.0],   # 6: nothing representable
                      [5.5, 5.5, 11.0, 11.0, 100.0]], np.float64)                  # 7: negative z clips at -1
    coords = [(-32767, 32767, -32767), (32767, -32767, 32767), (0, 0, 0), (1, 2, 3), (-1, -2, -3), (1023, 1025, 1),
              (7, 11, 13), (32767, 32767, 32767), (-32767, -32767, -32767), (100, 200, 50)]
    rows = np.array([(x, y, z, 1 + (i + j) % 4, i) for i in range(len(table)) for j, (x, y, z) in enumerate(coords)], np.int16)
    vp = np.arange(len(rows), dtype=np.int64)[::-1].copy()
    want = visible_ref(rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH)
    rel = want["pts"][:, 5:]
    assert (rel[:, 2] == 1).any() and (rel[:, 2] == -1).any() and (np.abs(rel[:, 0]) > 1e5).any() and (rel == 0).any()
    _assert_same(_run(cuda_device, rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH), want)
    _assert_same(_run(cuda_device, rows, vp, {i: tuple(r) for i, r in enumerate(table)}, P.CLASS_RULE_GOOGLE_EARTH), want, "dict")


@pytest.mark.parametrize("preset", ["GOOGLE_EARTH", "KITTI_360"])
def test_classes_and_scales_on_the_rule_boundaries(cuda_device, preset):
    rule = getattr(P, "CLASS_RULE_" + preset)
    bmin, bmax, cmin = 100, 10000, 10000      # the ranges of the two presets; GOOGLE_EARTH has no upper bound and no cars
    ids = [0, 1, 2, 5, 6, 7, 63, 64, 65, bmin - 1, bmin, bmin + 1, bmax - 2, bmax - 1, bmax, cmin - 1, cmin, cmin + 1, 16383,
           16384, 32766, 32767]
    ids = sorted(set(ids))
    rng = np.random.default_rng(5)
    rows = _random_rows(rng, 4 * len(ids), 1)
    rows[:, 4] = np.repeat(np.array(ids, np.int16), 4)[rng.permutation(len(rows))]
    table = np.full((32768, 5), np.nan)
    table[ids] = _random_table(rng, len(ids))
    vp = np.arange(len(rows), dtype=np.int64)
    want = visible_ref(rows, vp, table, rule)
    cls = dict(zip(want["pts"][:, 4].astype(int).tolist(), want["classes"].tolist()))
    assert cls[bmin - 1] == bmin - 1 and cls[bmin] == 2 and cls[bmin + 1] == 7 and cls[bmax - 1] == 7 and cls[5] == 5
    assert cls[bmax] == cls[32766] == (2 if preset == "GOOGLE_EARTH" else 3) and cls[32767] == (7 if preset == "GOOGLE_EARTH" else 3)
    special, plain = want["classes"] == 1, want["classes"] == 2      # ROAD is a special-z class in both, facade in neither
    assert special.any() and plain.any()
    assert (want["scales"][special, 2] == 1).all() and np.array_equal(want["scales"][plain, 2], want["scales"][plain, 0])
    assert want["instances"].tolist() == ids       # K spans ids below and above a 64-id word of the presence table
    _assert_same(_run(cuda_device, rows, vp, table, rule), want, preset)
    _assert_same(_run(cuda_device, rows, vp, table, rule, point_scale_factor=0.3), visible_ref(rows, vp, table, rule, 0.3), "factor")


def test_unknown_instances_raise_keyerror_only_when_visible(cuda_device):
    rng = np.random.default_rng(8)
    rows, table = _random_rows(rng, 500, 20), _random_table(rng, 24)
    table[21] = np.nan
    rows[100, 4], rows[200, 4], rows[300, 4] = 24, 21, -3      # past the table, a NaN row, negative
    rows[[5, 7, 9], 4] = 1, 2, 3
    vp = np.array([5, 100, 7, 200, 100, -1, 9], np.int64)
    t = [torch.from_numpy(a).to(cuda_device) for a in (rows, vp, table)]
    L = V.lib()
    nb = L.gcv_visible_workspace_bytes(500, len(vp))
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda_device)
    counts = (C.c_int64 * 3)()
    V.check(L.gcv_visible_count(t[1].data_ptr(), len(vp), t[0].data_ptr(), 500, t[2].data_ptr(), 24, ws.data_ptr(), nb, counts,
                                None), "gcv_visible_count")
    assert list(counts) == [5, 5, 2]
    with pytest.raises(KeyError, match=r"\[21, 24\]"):
        P.visible_point_set(*t, P.CLASS_RULE_GOOGLE_EARTH)
    with pytest.raises(KeyError):
        visible_ref(rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH)
    vp_neg = np.array([5, 300, 7], np.int64)
    with pytest.raises(KeyError, match=r"\[-3\]"):
        P.visible_point_set(t[0], torch.from_numpy(vp_neg).to(cuda_device), t[2], P.CLASS_RULE_GOOGLE_EARTH)
    vp_ok = np.array([5, 7, 9, 101, 199, 301], np.int64)        # the same rows exist, nobody sees them
    _assert_same(_run(cuda_device, rows, vp_ok, table, P.CLASS_RULE_GOOGLE_EARTH),
                 visible_ref(rows, vp_ok, table, P.CLASS_RULE_GOOGLE_EARTH))


class _Raw:
    """The C ABI by hand: outputs pre-filled with poison (NaN bit patterns / -1), `extra` slots longer than M."""

    def __init__(self, dev, rows, vp, table, rule=P.CLASS_RULE_GOOGLE_EARTH):
        self.L = V.lib()
        self.t = [torch.from_numpy(a).to(dev) for a in (rows, vp.reshape(-1), table)]
        self.n, self.npix, self.nc = len(rows), vp.size, len(table)
        self.nb = self.L.gcv_visible_workspace_bytes(self.n, self.npix)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=dev)
        self.rule, self.dev = P._native_rule(rule), dev
        self.a = (self.t[1].data_ptr(), self.npix, self.t[0].data_ptr(), self.n, self.t[2].data_ptr(), self.nc)

    def count(self):
        counts = (C.c_int64 * 3)(-9, -9, -9)
        rc = self.L.gcv_visible_count(*self.a, self.ws.data_ptr(), self.nb, counts, None)
        return rc, list(counts)

    def outputs(self, m, k, extra):
        f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=self.dev)   # noqa: E731
        return {"index": torch.full((m + extra,), -1, dtype=torch.int64, device=self.dev), "pts": f(m + extra, 8),
                "batch_idx": torch.full((m + extra,), -1, dtype=torch.int32, device=self.dev),
                "instances": torch.full((k + extra,), -1, dtype=torch.int16, device=self.dev), "classes": f(m + extra),
                "scales": f(m + extra, 3)}

    def emit(self, m, k, o, skip=()):
        ptr = lambda key: None if key in skip else o[key].data_ptr()   # noqa: E731
        rc = self.L.gcv_visible_emit(*self.a, C.byref(self.rule), self.ws.data_ptr(), self.nb, m, k, o["index"].data_ptr(),
                                     o["pts"].data_ptr(), ptr("batch_idx"), ptr("instances"), ptr("classes"), ptr("scales"), None)
        torch.cuda.synchronize()
        return rc


def _poison_left(t):
    return torch.isnan(t) if t.dtype == torch.float32 else t == -1


def test_poisoned_and_optional_outputs(cuda_device, random_case):
    rows, table, vp, want = random_case
    raw = _Raw(cuda_device, rows, vp, table)
    rc, (m, k, unknown) = raw.count()
    assert rc == 0 and (m, k, unknown) == (len(want["index"]), len(want["instances"]), 0)
    extra = 64
    o = raw.outputs(m, k, extra)
    assert raw.emit(m, k, o) == 0
    for key, t in o.items():
        n = k if key == "instances" else m
        assert not bool(_poison_left(t[:n]).any()), key          # every element of [0, M) written (no instance is -1 here)
        assert bool(_poison_left(t[n:]).all()), key              # nothing beyond M
        assert np.array_equal(_bits(t[:n].cpu().numpy().reshape(want[key].shape)), _bits(want[key])), key
    # NULL for the optional outputs: they stay poisoned, the two required ones come out the same
    for skip in (("batch_idx", "instances", "classes", "scales"), ("classes",), ("batch_idx", "scales"), ("instances",)):
        o2 = raw.outputs(m, k, extra)
        assert raw.emit(m, k, o2, skip=skip) == 0
        for key in o2:
            if key in skip:
                assert bool(_poison_left(o2[key]).all()), (skip, key)
            else:
                assert torch.equal(o2[key].view(torch.uint8), o[key].view(torch.uint8)), (skip, key)


def test_out_of_range_map_value_is_refused_and_never_used(cuda_device):
    rng = np.random.default_rng(4)
    n = 777
    rows, table = _random_rows(rng, n, 10), _random_table(rng, 10)
    for bad in (n, n + 1, 2 ** 31 + 5, 2 ** 62):
        vp = _random_map(rng, n, (8, 8), 20)
        vp[3, 3] = bad
        raw = _Raw(cuda_device, rows, vp, table)
        rc, counts = raw.count()
        assert rc == INVALID and b">= n_points" in raw.L.gcv_last_error() and counts == [-9, -9, -9]
        with pytest.raises(RuntimeError, match="gcv_status -1"):
            P.visible_point_set(raw.t[0], raw.t[1], raw.t[2], P.CLASS_RULE_GOOGLE_EARTH)
    # the value n - 1 is the last valid one
    vp[3, 3] = n - 1
    _assert_same(_run(cuda_device, rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH), visible_ref(rows, vp, table, P.CLASS_RULE_GOOGLE_EARTH))


def test_workspace_reuse_back_to_back(cuda_device, random_case):
    """Two different maps through one VisibleSetWorkspace on one stream, then the first again: every count starts from
    cleared marks, so no bit of the frame before survives."""
    rows, table, vp_a, want_a = random_case
    rng = np.random.default_rng(77)
    vp_b = _random_map(rng, N_RANDOM, (24, 40), 90)
    want_b = visible_ref(rows, vp_b, table, P.CLASS_RULE_GOOGLE_EARTH)
    assert not np.array_equal(want_a["index"], want_b["index"]) and len(want_b["instances"]) < len(want_a["instances"])
    ws = P.VisibleSetWorkspace(cuda_device)
    t_rows, t_tab = torch.from_numpy(rows).to(cuda_device), torch.from_numpy(table).to(cuda_device)
    maps = [torch.from_numpy(v).to(cuda_device) for v in (vp_a, vp_b, vp_a)]
    got = [P.visible_point_set(t_rows, v, t_tab, P.CLASS_RULE_GOOGLE_EARTH, workspace=ws) for v in maps]
    buf = ws.buf
    for g, w, name in zip(got, (want_a, want_b, want_a), "aba"):
        _assert_same(g, w, name)
    assert ws.buf is buf                                         # one allocation served the three frames
    # a smaller frame through the same (larger) workspace
    small = _random_rows(rng, 100, 300)
    vp_s = np.array([[99, 0, -1, 64]], np.int64)
    _assert_same(P.visible_point_set(torch.from_numpy(small).to(cuda_device), torch.from_numpy(vp_s).to(cuda_device), t_tab,
                                     P.CLASS_RULE_GOOGLE_EARTH, workspace=ws),
                 visible_ref(small, vp_s, table, P.CLASS_RULE_GOOGLE_EARTH), "small")
    assert ws.buf is buf


def test_end_to_end_on_the_synthetic_layout(cuda_device):
    """extrude_points -> visible_point_map -> visible_point_set on a 256 px layout, against visible_ref fed with the
    same rows and map copied to the host; ins_map is rows[:, 4][vp_map] on the visible pixels (inference.py:338)."""
    size = 256
    L = synth.s_layout(size, 2201, block=64, road=8, max_height=70)
    inv = {v: k for k, v in synth.LAYOUT_CLASSES.items()}
    maps = [torch.from_numpy(L[k]).to(cuda_device) for k in ("INS", "TD_HF", "BU_HF", "PTS")]
    rows = P.extrude_points(True, inv, synth.LAYOUT_SCALES, synth.LAYOUT_SEG_INS, *maps)
    rig, cam_pos, cam_quat = synth.layout_camera(size, W=240, H=136)
    vp_map, ins_map = P.visible_point_map(rows, rig, cam_pos.copy(), cam_quat, 0)
    rows_h, vp_h = rows.cpu().numpy(), vp_map.cpu().numpy()
    centers = {}
    for ins in np.unique(rows_h[:, 4]):       # a box per instance, as CENTERS.pkl holds one: centre and extents
        p = rows_h[rows_h[:, 4] == ins][:, :3].astype(np.float64)
        lo, hi = p.min(0), p.max(0)
        centers[int(ins)] = ((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[0] - lo[0], hi[1] - lo[1], hi[2])
    want = visible_ref(rows_h, vp_h, centers, P.CLASS_RULE_GOOGLE_EARTH)
    # (not a degenerate frame: hundreds of points of several instances, facades and roofs among them)
    assert len(want["index"]) > 500 and len(want["instances"]) > 5 and {2.0, 7.0} <= set(want["classes"].tolist())
    got = P.visible_point_set(rows, vp_map, centers, P.CLASS_RULE_GOOGLE_EARTH)
    _assert_same(got, want)
    seen = vp_h >= 0
    assert seen.mean() > 0.5 and np.array_equal(ins_map.cpu().numpy()[seen], rows_h[:, 4][vp_h][seen])
