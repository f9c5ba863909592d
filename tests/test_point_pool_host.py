"""SerializedPooling / SerializedUnpooling over the library (include/gcs.h, gaussiancity_amd/point_pool.py), the part that
needs no GPU: the numpy formulation of the plan against the fixture recorded from models/pt_v3.py on the CPU, the exports
and the capability query, the workspace query, every refusal before a HIP call, and install() / uninstall() on a stand-in
module."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import pool_ref as R
from gaussiancity_amd import _native_s as S
from gaussiancity_amd import point_pool as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SYMBOLS = ("gcs_pool_reduces", "gcs_pool_plan_workspace_bytes", "gcs_pool_plan_count", "gcs_pool_plan_emit",
           "gcs_segment_gather_forward_t", "gcs_segment_gather_backward_t", "gcs_segment_expand_add_t")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_pool.npz"))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_reference_plan_equals_the_golden(golden, case):
    """Every integer key of the reference's pooled point set, from the input codes alone.  The recorded run's sorts are
    stable, which is what makes `head` (grid_coord, batch, the codes) comparable at all."""
    g = lambda k: golden["%s.int.%s" % (case, k)]  # noqa: E731
    stride, depth = int(golden[case + ".stride"]), int(g("in.serialized_depth"))
    d = (math.ceil(stride) - 1).bit_length()
    d = 0 if d > depth else d
    assert d == {"a": 1, "b": 1, "c": 0}[case]
    p = R.plan(g("in.serialized_code"), 3 * d)
    assert p.n == 333 and p.s == g("batch").shape[0] and 1 < p.s < p.n
    assert np.array_equal(p.cluster, g("pooling_inverse"))
    assert np.array_equal(p.code, g("serialized_code"))
    assert np.array_equal(p.order, g("serialized_order"))
    assert np.array_equal(p.inverse, g("serialized_inverse"))
    assert np.array_equal(golden[case + ".grid"][p.head] >> d, g("grid_coord"))
    assert np.array_equal(golden["batch"][p.head], g("batch"))
    assert int(g("serialized_depth")) == depth - d
    assert np.array_equal(p.idx_ptr[1:], np.cumsum(np.bincount(p.cluster)))
    assert (np.diff(p.idx_ptr) > 1).any()   # clusters of several rows: the head choice matters


def test_reference_ties_go_to_the_lower_row_and_keys_are_signed():
    code = np.array([[9, -8, 9, 1, -8, 1 << 50], [5, 5, 7, 5, 0, 5]], np.int64)
    p = R.plan(code, 3)
    assert p.cluster.tolist() == [2, 0, 2, 1, 0, 3] and p.s == 4   # keys 1, -1, 1, 0, -1, 2^47
    assert p.indices.tolist() == [1, 4, 3, 0, 2, 5] and p.idx_ptr.tolist() == [0, 2, 3, 5, 6] and p.head.tolist() == [1, 3, 0, 5]
    assert p.code.tolist() == [[-1, 0, 1, 1 << 47], [0, 0, 0, 0]]
    assert p.order.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]] and p.inverse.tolist() == p.order.tolist()


def test_new_symbols_are_exported_and_abi_stays_4():
    lib = S.lib()
    header = open(os.path.join(ROOT, "include", "gcs.h")).read()
    for name in SYMBOLS:
        assert name in S.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.gcs_abi_version() == 4 == S.ABI_VERSION == int(re.search(r"#define GCS_ABI_VERSION (\d+)", header).group(1))
    assert lib.gcs_pool_reduces() == 15
    assert PP.reduces() == PP.REDUCES == ("sum", "mean", "min", "max")


def test_workspace_query_is_monotone_and_range_checked():
    lib = S.lib()
    ns = (1, 2, 4095, 4096, 4097, 150_000, 2 ** 31 - 1)
    for k in range(1, 6):
        sizes = [lib.gcs_pool_plan_workspace_bytes(n, k) for n in ns]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    for n in ns:
        sizes = [lib.gcs_pool_plan_workspace_bytes(n, k) for k in range(1, 6)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    for n, k, word in ((0, 1, b"n must"), (-1, 1, b"n must"), (2 ** 31, 1, b"n must"), (10, 0, b"k must"), (10, 6, b"k must")):
        lib.gcs_subm_plan(0, 0, 0, 0, None)  # (another text first)
        assert lib.gcs_pool_plan_workspace_bytes(n, k) == 0
        err = lib.gcs_last_error()
        assert b"gcs_pool_plan_workspace_bytes" in err and word in err


def _host_args():
    """Host memory in the roles of the device buffers: every call below fails a check before anything is read."""
    buf = (C.c_double * 4096)()
    return buf, (C.addressof(buf) + 255) // 256 * 256


def test_plan_refusals_come_back_before_any_hip_call():
    lib = S.lib()
    buf, p = _host_args()
    need = lib.gcs_pool_plan_workspace_bytes(1000, 3)
    counts = (C.c_int64 * 1)(-7)

    def count(code=p, k=3, n=1000, shift=3, ws=p, wsb=need, out=counts):
        return lib.gcs_pool_plan_count(code, k, n, shift, ws, wsb, out, None)

    def emit(code=p, k=3, n=1000, shift=3, s=500, ws=p, wsb=need, cluster=p, indices=p, idx_ptr=p, head=p, dcode=p, dorder=p,
             dinv=p):
        return lib.gcs_pool_plan_emit(code, k, n, shift, s, ws, wsb, cluster, indices, idx_ptr, head, dcode, dorder, dinv, None)

    shared = [(dict(n=0), b"n must"), (dict(n=-5), b"n must"), (dict(n=2 ** 31), b"n must"), (dict(k=0), b"k must"),
              (dict(k=6), b"k must"), (dict(shift=-3), b"shift"), (dict(shift=51), b"shift"), (dict(shift=4), b"shift"),
              (dict(code=None), b"code"), (dict(ws=None), b"workspace"), (dict(wsb=need - 1), b"workspace"),
              (dict(wsb=0), b"workspace")]
    for fn, who in ((count, b"gcs_pool_plan_count"), (emit, b"gcs_pool_plan_emit")):
        for kw, word in shared:
            lib.gcs_subm_plan(0, 0, 0, 0, None)  # (some other error text first)
            assert fn(**kw) == INVALID, kw
            err = lib.gcs_last_error()
            assert who in err and word in err, (kw, err)
    # the pinned word: null, and host memory that the device cannot write
    assert count(out=None) == INVALID and b"counts_host" in lib.gcs_last_error()
    assert count() == INVALID and b"counts_host" in lib.gcs_last_error() and list(counts) == [-7]
    for kw, word in ((dict(s=0), b"s is not"), (dict(s=1001), b"s is not"), (dict(s=-1), b"s is not"),
                     (dict(cluster=None), b"cluster"), (dict(indices=None), b"indices"), (dict(idx_ptr=None), b"idx_ptr"),
                     (dict(head=None), b"head"), (dict(dcode=None), b"down_code"), (dict(dorder=None), b"down_order"),
                     (dict(dinv=None), b"down_inverse")):
        assert emit(**kw) == INVALID, kw
        assert word in lib.gcs_last_error(), kw
    # shift 48 and 0, and s = 1 and s = n, pass those checks (and fail the next one asked for)
    assert emit(shift=48, s=1, cluster=None) == INVALID and b"cluster" in lib.gcs_last_error()
    assert emit(shift=0, s=1000, ws=None) == INVALID and b"workspace" in lib.gcs_last_error()
    with pytest.raises(RuntimeError, match="gcs_status -1"):
        S.check(count(k=0), "gcs_pool_plan_count")


def test_gather_refusals_come_back_before_any_hip_call():
    lib = S.lib()
    buf, p = _host_args()

    def fwd(dtype=0, src=p, stride=32, m=100, f=32, indices=p, indptr=p, s=10, reduce=0, out=p, arg=None):
        return lib.gcs_segment_gather_forward_t(dtype, src, stride, m, f, indices, indptr, s, reduce, out, arg, None)

    def bwd(dtype=0, dout=p, m=100, f=32, cluster=p, indptr=p, s=10, reduce=0, arg=None, dsrc=p, stride=32):
        return lib.gcs_segment_gather_backward_t(dtype, dout, m, f, cluster, indptr, s, reduce, arg, dsrc, stride, None)

    def add(dtype=0, a=p, b=p, cluster=p, m=100, f=32, out=p):
        return lib.gcs_segment_expand_add_t(dtype, a, b, cluster, m, f, out, None)

    common = [(dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(m=0), b"sizes"), (dict(f=0), b"sizes"),
              (dict(m=2 ** 31), b"sizes"), (dict(f=2 ** 31), b"sizes")]
    cases = {fwd: common + [(dict(s=0), b"sizes"), (dict(stride=31), b"stride"), (dict(reduce=4), b"reduce"),
                            (dict(reduce=-1), b"reduce"), (dict(src=None), b"null"), (dict(out=None), b"null"),
                            (dict(indices=None), b"index pointer"), (dict(indptr=None), b"index pointer"),
                            (dict(indptr=p + 4), b"index pointer"), (dict(reduce=3), b"arg"), (dict(reduce=2), b"arg"),
                            (dict(dtype=1, src=p + 1), b"aligned"), (dict(src=p + 2), b"aligned")],
             bwd: common + [(dict(s=0), b"sizes"), (dict(stride=31), b"stride"), (dict(reduce=4), b"reduce"),
                            (dict(dout=None), b"null"), (dict(dsrc=None), b"null"), (dict(cluster=None), b"index pointer"),
                            (dict(indptr=None), b"index pointer"), (dict(reduce=3), b"arg"), (dict(dtype=1, dsrc=p + 1), b"aligned")],
             add: common + [(dict(b=None), b"null"), (dict(out=None), b"null"), (dict(cluster=None), b"index pointer"),
                            (dict(a=p + 2), b"aligned"), (dict(dtype=1, b=p + 1), b"aligned")]}
    names = {fwd: b"gcs_segment_gather_forward_t", bwd: b"gcs_segment_gather_backward_t", add: b"gcs_segment_expand_add_t"}
    for fn, rows in cases.items():
        for kw, word in rows:
            lib.gcs_subm_plan(0, 0, 0, 0, None)  # (some other error text first)
            assert fn(**kw) == INVALID, (names[fn], kw)
            err = lib.gcs_last_error()
            assert names[fn] in err and word in err, (kw, err)


def _cpu_plan():
    p = R.plan(np.array([[3, 1, 3, 0]], np.int64), 0)
    return PP.PoolPlan(*[torch.from_numpy(np.ascontiguousarray(v)) for v in p[:7]], p.n, p.s)


def test_python_layer_refuses_cpu_tensors_and_unknown_reduces():
    plan = _cpu_plan()
    with pytest.raises(ValueError, match="CUDA tensor"):
        PP.pool_plan(torch.zeros(2, 4, dtype=torch.int64), 1)
    with pytest.raises(ValueError, match="CUDA tensor"):
        PP.pooled_reduce(torch.zeros(4, 8), plan, "sum")
    with pytest.raises(ValueError, match="CUDA tensor"):
        PP.unpool_add(torch.zeros(4, 8), torch.zeros(3, 8), plan)
    src = torch.zeros(4, 8, device="meta")  # is_cuda is False: refused in the same way, before anything is called
    with pytest.raises(ValueError, match="CUDA tensor"):
        PP.pooled_reduce(src, plan, "median")
    assert set(PP.stats()) == {"plan_calls", "reduce_calls", "reduce_backward_calls", "unpool_calls", "pooling_fused",
                               "pooling_original", "unpooling_fused", "unpooling_original"}
    assert PP.FIELDS == ("cluster", "indices", "idx_ptr", "head", "code", "order", "inverse", "n", "s") == R.Plan._fields


def test_unknown_reduce_is_refused():
    """The reduce is checked after the device: with a tensor that says it is a CUDA tensor, 'median' is a ValueError."""
    plan = _cpu_plan()

    class Fake(torch.Tensor):
        is_cuda = True

    src = torch.zeros(4, 8).as_subclass(Fake)
    with pytest.raises(ValueError, match="reduce must be one of sum, mean, min, max"):
        PP.pooled_reduce(src, plan, "median")


class _Dict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stand_in():
    """A module in the shape of models/pt_v3.py: the three classes, whose methods record their calls."""
    calls = []

    class Point(_Dict):
        pass

    class SerializedPooling:
        stride, reduce, shuffle_orders, traceable = 2, "max", True, True
        proj = types.SimpleNamespace(weight=torch.zeros(4, 4))

        def forward(self, point):
            calls.append(("pooling", id(point)))
            return "pooled"

    class SerializedUnpooling:
        traceable = False

        def forward(self, point):
            calls.append(("unpooling", id(point)))
            return "unpooled"

    return types.SimpleNamespace(Point=Point, SerializedPooling=SerializedPooling, SerializedUnpooling=SerializedUnpooling), calls


def test_install_rebinds_uninstall_restores_and_cpu_tensors_reach_the_originals():
    M, calls = _stand_in()
    own = (M.SerializedPooling.forward, M.SerializedUnpooling.forward)
    PP.install(M)
    rebound = (M.SerializedPooling.forward, M.SerializedUnpooling.forward)
    assert rebound[0] is not own[0] and rebound[1] is not own[1]
    PP.install(M)   # a second install changes nothing
    assert (M.SerializedPooling.forward, M.SerializedUnpooling.forward) == rebound
    PP.reset_stats()
    point = M.Point(feat=torch.zeros(5, 4), coord=torch.zeros(5, 3), grid_coord=torch.zeros(5, 3, dtype=torch.int32),
                    batch=torch.zeros(5, dtype=torch.long), serialized_code=torch.zeros(1, 5, dtype=torch.long),
                    serialized_order=torch.zeros(1, 5, dtype=torch.long), serialized_inverse=torch.zeros(1, 5, dtype=torch.long),
                    serialized_depth=3)
    assert M.SerializedPooling().forward(point) == "pooled" and calls == [("pooling", id(point))]
    with pytest.raises(AssertionError, match="Run point.serialization"):
        M.SerializedPooling().forward(M.Point(serialized_depth=3))   # upstream's assertion comes first
    child = M.Point(feat=torch.zeros(2, 4), pooling_parent=point, pooling_inverse=torch.zeros(5, dtype=torch.long))
    assert M.SerializedUnpooling().forward(child) == "unpooled" and calls[-1] == ("unpooling", id(child))
    assert "pooling_parent" in child   # without a plan the original method gets the point untouched
    with pytest.raises(AssertionError):
        M.SerializedUnpooling().forward(M.Point(feat=torch.zeros(2, 4)))
    st = PP.stats()
    assert st["pooling_original"] == 1 and st["unpooling_original"] == 1 and st["pooling_fused"] == st["unpooling_fused"] == 0
    assert st["plan_calls"] == st["reduce_calls"] == st["unpool_calls"] == 0
    PP.uninstall(M)
    assert (M.SerializedPooling.forward, M.SerializedUnpooling.forward) == own
    PP.uninstall(M)  # nothing installed: nothing to do
    assert (M.SerializedPooling.forward, M.SerializedUnpooling.forward) == own
