"""Index plans of the point backbone (include/gcs.h, gaussiancity_amd/point_index.py), the part that needs no GPU: the
numpy formulation against the fixture recorded from models/pt_v3.py on the CPU, the exports and the capability query,
the workspace query, every refusal before a HIP call, and install() / uninstall() on a stand-in module."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import index_ref as R
from gaussiancity_amd import _native_s as S
from gaussiancity_amd import point_index as PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
DEPTHS = (1, 5, 8, 11, 16)
PLANS = ("p4", "p1024", "p16", "p32", "one", "zero")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ptv3_index.npz"))


@pytest.mark.parametrize("with_batch", [0, 1])
@pytest.mark.parametrize("depth", DEPTHS)
def test_reference_codes_equal_the_golden(golden, depth, with_batch):
    g, b = golden["d%d.grid" % depth], golden["d%d.batch" % depth]
    want = golden["d%d.code.%d" % (depth, with_batch)]
    assert want.shape == (5, 97) and want.dtype == np.int64
    got = R.codes(g, b if with_batch else None, depth, R.ORDERS)
    for r, name in enumerate(R.ORDERS):
        assert np.array_equal(got[r], want[r]), name


def test_reference_cord_divides_as_the_golden(golden):
    """grid_size 0.003 with coordinates up to 511, and every coordinate below 256 at 0.01: the binary32 division."""
    assert np.array_equal(R.codes(golden["cord003.grid"], None, 9, ("cord",), 0.003), golden["cord003.code"])
    assert int(golden["cord003.grid"].max()) == 511
    assert np.array_equal(R.codes(golden["cord256.grid"], None, 8, ("cord",), 0.01), golden["cord256.code"])


@pytest.mark.parametrize("name", PLANS)
def test_reference_patch_plan_equals_the_golden(golden, name):
    pad, unpad, cu = R.patch_plan(np.cumsum(golden[name + ".counts"]), int(golden[name + ".patch"]))
    for got, key in ((pad, "pad"), (unpad, "unpad"), (cu, "cu")):
        want = golden["%s.%s" % (name, key)]
        assert got.dtype == want.dtype and np.array_equal(got, want), key


def test_reference_order_is_stable_and_signed():
    code = np.array([[3, -1, 3, 0, -1, 1 << 62]], np.int64)
    order, inverse = R.order_inverse(code)
    assert order.tolist() == [[1, 4, 3, 0, 2, 5]] and inverse[0, order[0]].tolist() == list(range(6))


def test_new_symbols_are_exported_and_abi_stays_4():
    lib = S.lib()
    for name in ("gcs_index_orders", "gcs_serialize_workspace_bytes", "gcs_serialize", "gcs_patch_plan_count",
                 "gcs_patch_plan_emit"):
        assert name in S.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    header = open(os.path.join(ROOT, "include", "gcs.h")).read()
    assert lib.gcs_abi_version() == 4 == S.ABI_VERSION == int(re.search(r"#define GCS_ABI_VERSION (\d+)", header).group(1))
    assert lib.gcs_index_orders() == 31
    assert PI.orders() == PI.ORDERS == R.ORDERS == tuple(S.ORDERS)
    for name, value in S.ORDERS.items():
        enum = "GCS_ORDER_" + name.upper().replace("-", "_")
        assert re.search(r"\b%s = %d\b" % (enum, value), header), enum


def test_workspace_query_is_monotone_and_range_checked():
    lib = S.lib()
    ns = (0, 1, 4095, 4096, 4097, 100_003, 2 ** 31 - 1)
    for k in range(1, 6):
        sizes = [lib.gcs_serialize_workspace_bytes(n, k) for n in ns]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    for n in ns:
        sizes = [lib.gcs_serialize_workspace_bytes(n, k) for k in range(1, 6)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.gcs_serialize_workspace_bytes(100_003, 4) < 64 * 100_003   # a few words a point and order, no key copies
    for n, k, word in ((-1, 1, b"n must"), (2 ** 31, 1, b"n must"), (10, 0, b"n_orders"), (10, 6, b"n_orders")):
        lib.gcs_serialize(None, None, 0, 0, 0, 1.0, 1.0, None, 1, None, None, None, None, 0, None)  # (another text first)
        assert lib.gcs_serialize_workspace_bytes(n, k) == 0
        err = lib.gcs_last_error()
        assert b"gcs_serialize_workspace_bytes" in err and word in err


def _host_args():
    """Host memory in the roles of the device buffers: every call below fails a check before anything is read."""
    buf = (C.c_double * 4096)()
    return buf, (C.addressof(buf) + 255) // 256 * 256


def _orders(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def test_serialize_refusals_come_back_before_any_hip_call():
    lib = S.lib()
    buf, p = _host_args()
    need = lib.gcs_serialize_workspace_bytes(1000, 2)

    def call(coord=p, batch=p, n=1000, nb=57, depth=8, dx=1e-4, dy=1e-2, orders=_orders(0, 3), k=2, code=p, order=p, inv=p,
             ws=p, wsb=need):
        return lib.gcs_serialize(coord, batch, n, nb, depth, dx, dy, orders, k, code, order, inv, ws, wsb, None)

    cases = [(dict(depth=0), b"depth"), (dict(depth=17), b"depth"), (dict(depth=-3), b"depth"),
             (dict(depth=16, nb=2 ** 15), b"bit_length(n_batches)"), (dict(depth=16, nb=2 ** 31 - 1), b"bit_length(n_batches)"),
             (dict(nb=0), b"n_batches"),
             (dict(orders=_orders(0, 5)), b"unknown order"), (dict(orders=_orders(-1, 0)), b"unknown order"),
             (dict(orders=_orders(3, 3)), b"repeated order"), (dict(orders=None), b"orders_host"),
             (dict(k=0), b"n_orders"), (dict(k=6), b"n_orders"), (dict(k=-1), b"n_orders"),
             (dict(ws=None), b"workspace"), (dict(wsb=need - 1), b"workspace"), (dict(wsb=0), b"workspace"),
             (dict(n=-1), b"n must"), (dict(n=2 ** 31), b"n must"),
             (dict(dx=0.0), b"cord_div_x"), (dict(dy=float("nan")), b"cord_div_y"),
             (dict(coord=None), b"grid_coord"), (dict(code=None), b"code"), (dict(order=None), b"order"),
             (dict(inv=None), b"inverse")]
    for kw, word in cases:
        lib.gcs_subm_plan(0, 0, 0, 0, None)  # (some other error text first)
        assert call(**kw) == INVALID, kw
        err = lib.gcs_last_error()
        assert b"gcs_serialize" in err and word in err, (kw, err)
    # 16 * 3 + bit_length(2^15 - 1) = 63 bits pass that check (and fail the next one asked for: the workspace)
    assert call(depth=16, nb=2 ** 15 - 1, ws=None) == INVALID and b"workspace" in lib.gcs_last_error()
    # no points: nothing to do, nothing is read or queued
    assert call(n=0, coord=None, batch=None, code=None, order=None, inv=None) == 0
    with pytest.raises(RuntimeError, match="gcs_status -1"):
        S.check(call(depth=0), "gcs_serialize")


def test_patch_plan_refusals_come_back_before_any_hip_call():
    lib = S.lib()
    buf, p = _host_args()
    counts = (C.c_int64 * 2)(-7, -7)

    def count(off=p, nb=57, P=1024, out=counts):
        return lib.gcs_patch_plan_count(off, nb, P, out, None)

    def emit(off=p, nb=57, P=1024, padded=5000, n_cu=62, pad=p, unpad=p, cu=p):
        return lib.gcs_patch_plan_emit(off, nb, P, padded, n_cu, pad, unpad, cu, None)

    for fn, who in ((count, b"gcs_patch_plan_count"), (emit, b"gcs_patch_plan_emit")):
        for kw, word in ((dict(nb=0), b"n_batches"), (dict(nb=-1), b"n_batches"), (dict(P=0), b"patch_size"),
                         (dict(P=-4), b"patch_size"), (dict(off=None), b"offset")):
            assert fn(**kw) == INVALID, kw
            err = lib.gcs_last_error()
            assert who in err and word in err, (kw, err)
    assert count(out=None) == INVALID and b"counts_host" in lib.gcs_last_error()
    assert list(counts) == [-7, -7]
    for kw, word in ((dict(padded=-1), b"padded"), (dict(padded=2 ** 31), b"padded"), (dict(n_cu=0), b"n_cu"),
                     (dict(n_cu=5000 + 57 + 2), b"n_cu"), (dict(pad=None), b"pad"), (dict(unpad=None), b"unpad"),
                     (dict(cu=None), b"cu_seqlens")):
        assert emit(**kw) == INVALID, kw
        assert word in lib.gcs_last_error(), kw


def test_python_layer_refuses_cpu_tensors_and_unknown_orders():
    g = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA tensor"):
        PI.serialize(g, None, 8, ("z",))
    with pytest.raises(ValueError, match="CUDA tensor"):
        PI.patch_plan(torch.tensor([4]), 4)
    assert set(PI.stats()) == {"serialize_calls", "patch_plan_calls"}


class _Dict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stand_in():
    """A module in the shape of models/pt_v3.py: the two classes, whose methods record their calls."""
    calls = []

    class Point(_Dict):
        def serialization(self, order="z", depth=None, shuffle_orders=False):
            calls.append(("serialization", tuple(order), depth, shuffle_orders))
            self["serialized_depth"] = "original"

    class SerializedAttention:
        patch_size = 4

        def get_padding_and_inverse(self, point):
            calls.append(("get_padding_and_inverse",))
            return "pad", "unpad", "cu"

    return types.SimpleNamespace(Point=Point, SerializedAttention=SerializedAttention), calls


def test_install_rebinds_uninstall_restores_and_cpu_tensors_reach_the_originals():
    M, calls = _stand_in()
    own = (M.Point.serialization, M.SerializedAttention.get_padding_and_inverse)
    PI.install(M)
    rebound = (M.Point.serialization, M.SerializedAttention.get_padding_and_inverse)
    assert rebound[0] is not own[0] and rebound[1] is not own[1]
    PI.install(M)   # a second install changes nothing
    assert (M.Point.serialization, M.SerializedAttention.get_padding_and_inverse) == rebound
    PI.reset_stats()
    point = M.Point(grid_coord=torch.zeros(5, 3, dtype=torch.int32), batch=torch.zeros(5, dtype=torch.long),
                    offset=torch.tensor([5]))
    point.serialization(order=["z", "hilbert"], shuffle_orders=True)
    assert calls == [("serialization", ("z", "hilbert"), None, True)] and point["serialized_depth"] == "original"
    assert M.SerializedAttention().get_padding_and_inverse(point) == ("pad", "unpad", "cu")
    assert calls[-1] == ("get_padding_and_inverse",)
    # cached keys are returned as they are, without the original and without the library
    point["pad"], point["unpad"], point["cu_seqlens_key"] = 1, 2, 3
    assert M.SerializedAttention().get_padding_and_inverse(point) == (1, 2, 3) and len(calls) == 2
    with pytest.raises(AssertionError):
        M.Point(grid_coord=torch.zeros(5, 3, dtype=torch.int32)).serialization()   # upstream's `"batch" in self.keys()`
    assert PI.stats() == {"serialize_calls": 0, "patch_plan_calls": 0}
    PI.uninstall(M)
    assert (M.Point.serialization, M.SerializedAttention.get_padding_and_inverse) == own
    PI.uninstall(M)  # nothing installed: nothing to do
    assert (M.Point.serialization, M.SerializedAttention.get_padding_and_inverse) == own
