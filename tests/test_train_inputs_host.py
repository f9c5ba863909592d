"""-m "not gpu": the host side of gaussiancity_amd.train_inputs (include/gcv.h K23 / K24).  The restatement the GPU tests use
(tests/train_inputs_ref.py) reproduces what the reference's own lines recorded (tests/golden/train_inputs.npz, written by
tests/golden/make_train_inputs_golden.py) bit for bit, the codes and the generator's end state included; rule_from_cfg
reads config.py's values; every argument error of the four entry points comes back through the loaded library before
anything is queued; install / uninstall restore the function."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import train_inputs_ref as R
from gaussiancity_amd import _native_v as V
from gaussiancity_amd import train_inputs as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_inputs.npz")
CASES = ["%s/z%s" % (d, z) for d in ("ge", "ki") for z in ("256", "8", "none")]
RULES = {"ge": T.RULE_GOOGLE_EARTH, "ki": T.RULE_KITTI_360}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_case(golden, name):
    """(pts, rule, z_dim, proj_tlp) of a recorded case."""
    short = name.split("/")[0]
    z_dim = int(golden[name + "/z_dim"])
    tlp = golden[name + "/tlp"]
    return (torch.from_numpy(golden[short + "/pts"]), RULES[short](float(golden["scale_factor"])), None if z_dim < 0 else z_dim,
            None if tlp.shape[0] == 0 else torch.from_numpy(tlp))


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_recorded_results(golden, name):
    pts, rule, z_dim, tlp = golden_case(golden, name)
    torch.set_rng_state(torch.from_numpy(golden["rng_before"]))
    got = R.restate(pts, rule, z_dim, tlp)
    assert got["flagged"] == 0
    for k in ("bch_idx", "classes", "scales", "onehots", "proj_uv"):
        want = torch.from_numpy(golden[name + "/" + k])
        assert got[k].dtype == want.dtype and got[k].shape == want.shape and torch.equal(got[k], want), k
        assert np.array_equal(got[k].numpy().view(np.uint8), want.numpy().view(np.uint8)), k
    if z_dim is None:
        assert torch.equal(torch.get_rng_state(), torch.from_numpy(golden["rng_before"]))
        return
    assert got["z_keys"] == golden[name + "/z_keys"].tolist()
    assert np.array_equal(got["z_codes"].numpy().view(np.uint32), golden[name + "/z_codes"].view(np.uint32))
    assert np.array_equal(np.packbits(got["z_idx"].numpy(), axis=1), golden[name + "/z_idx"])
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(golden[name + "/rng_after"]))
    group, ids = R.groups(pts, rule)
    assert ids.tolist() == got["z_keys"] and torch.equal(group.long(), got["z_idx"].long().argmax(0))
    assert torch.equal(group.long(), got["bch_idx"][0])       # NormalizePointCords numbers the instances the same way


def test_the_fixture_covers_the_rules_edges(golden):
    for short, rule in (("ge", T.RULE_GOOGLE_EARTH()), ("ki", T.RULE_KITTI_360())):
        ids = set(golden[short + "/pts"][0, :, 4].astype(int).tolist())
        assert {rule.bldg_ins_min, rule.bldg_ins_min + 1, rule.bldg_ins_max - 2, rule.bldg_ins_max - 1} <= ids
        assert set(rule.special_z_classes) <= ids
        if rule.car_ins_max > rule.car_ins_min:
            assert {rule.car_ins_min, rule.car_ins_max - 1} <= ids
    assert os.path.getsize(GOLDEN) < 100 * 1024


def _cfg_node(golden, dataset):
    node = types.SimpleNamespace()
    for key in golden.files:
        parts = key.split("/")
        if parts[0] == "cfg" and parts[1] == dataset and parts[2] != "Z_SCALE_SPECIAL_CLASSES":
            v = golden[key]
            setattr(node, parts[2], v.tolist())
    special = golden["cfg/%s/Z_SCALE_SPECIAL_CLASSES" % dataset].tolist()
    node.Z_SCALE_SPECIAL_CLASSES = {"NAME_%d" % c: c for c in reversed(special)}
    return node


def test_rule_from_cfg_reads_config_pys_values(golden):
    f = float(golden["scale_factor"])
    ge, ki = _cfg_node(golden, "GOOGLE_EARTH"), _cfg_node(golden, "KITTI_360")
    assert not hasattr(ge, "CAR_RANGE") and ki.CAR_RANGE == [10000, 16384]
    assert T.rule_from_cfg(ge, f) == T.RULE_GOOGLE_EARTH(f) == T.RULE_GOOGLE_EARTH()
    assert T.rule_from_cfg(ki, f) == T.RULE_KITTI_360(f) == T.RULE_KITTI_360()
    assert T.RULE_GOOGLE_EARTH() == T.TrainRule(100, 32768, 0, 0, 2, 7, 0, 8, (1, 5, 6), 0.65, 2048.0)
    assert T.RULE_KITTI_360() == T.TrainRule(100, 10000, 10000, 16384, 2, 7, 3, 8, (1, 6), 0.65, 2048.0)
    native = T._native_rule(T.RULE_KITTI_360())
    assert native.special_z_classes == (1 << 1) | (1 << 6) and native.car_ins_max == 16384 and native.n_classes == 8
    assert native.scale_factor == np.float32(0.65) and native.proj_size == 2048.0
    for bad in (T.RULE_KITTI_360()._replace(n_classes=0), T.RULE_KITTI_360()._replace(n_classes=33),
                T.RULE_KITTI_360()._replace(special_z_classes=(32,))):
        with pytest.raises(ValueError):
            T._native_rule(bad)


def test_the_new_symbols_are_exported_and_declared():
    L = V.lib()
    names = ("gcv_train_inputs_max_classes", "gcv_train_inputs_workspace_bytes", "gcv_train_inputs_count", "gcv_train_inputs_emit")
    assert all(n in V.EXPORTED_SYMBOLS and hasattr(L, n) for n in names)
    assert all(n.replace("_", "").isalpha() for n in names)
    assert L.gcv_train_inputs_max_classes() == 32
    assert L.gcv_abi_version() == V.ABI_VERSION == 5
    assert C.sizeof(V.TrainRule) == 44
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcv.h")).read()
    assert all(n + "(" in header for n in names)
    assert "#define GCV_TRAIN_INPUTS_FLAG_OFFSET %d\n" % V.TRAIN_INPUTS_FLAG_OFFSET in header


def test_workspace_bytes():
    L = V.lib()
    n = L.gcv_train_inputs_workspace_bytes(16384)
    assert n >= 2 * 4096 + 12 and n % 16 == 0 and n == L.gcv_train_inputs_workspace_bytes(0) == L.gcv_train_inputs_workspace_bytes(2 ** 31 - 1)
    for bad in (-1, 2 ** 31):
        assert L.gcv_train_inputs_workspace_bytes(bad) == 0
        assert b"n_rows" in L.gcv_last_error()


def _rule(**kw):
    r = T._native_rule(T.RULE_KITTI_360())
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_argument_errors_come_back_before_anything_is_queued():
    """No GPU here: a call that got as far as queueing would fail with a HIP error (gcv_status -2), and the pointers are
    made-up addresses that nothing may dereference."""
    L = V.lib()
    nbytes = L.gcv_train_inputs_workspace_bytes(64)
    pts, ws, out = 0x10000, 0x20000, 0x30000
    counts = (C.c_int64 * 2)(-7, -7)

    def count(p=pts, stride=9, n=64, w=ws, wb=nbytes, c=counts):
        return L.gcv_train_inputs_count(p, stride, n, w, wb, c, None)

    def emit(p=pts, stride=9, n=64, per=64, rule=None, tlp=None, w=ws, wb=nbytes, groups=0, n_ins=0, outs=(out,) * 5,
             group=None, ids=None, null_rule=False):
        rule = rule if rule is not None else _rule()
        return L.gcv_train_inputs_emit(p, stride, n, per, None if null_rule else C.byref(rule), tlp, w, wb, groups, n_ins, *outs,
                                       group, ids, None)

    bad_calls = {
        "count: null pts": lambda: count(p=None), "count: misaligned pts": lambda: count(p=pts + 2),
        "count: row_stride 8": lambda: count(stride=8), "count: negative n_rows": lambda: count(n=-1),
        "count: n_rows 2^31": lambda: count(n=2 ** 31), "count: null workspace": lambda: count(w=None),
        "count: misaligned workspace": lambda: count(w=ws + 8), "count: short workspace": lambda: count(wb=nbytes - 1),
        "count: null counts_host": lambda: count(c=None),
        "emit: null pts": lambda: emit(p=None), "emit: misaligned pts": lambda: emit(p=pts + 1),
        "emit: row_stride 8": lambda: emit(stride=8), "emit: negative n_rows": lambda: emit(n=-1, per=1),
        "emit: n_rows 2^31": lambda: emit(n=2 ** 31, per=2 ** 31), "emit: null workspace": lambda: emit(w=None),
        "emit: misaligned workspace": lambda: emit(w=ws + 4), "emit: short workspace": lambda: emit(wb=nbytes - 1),
        "emit: null rule": lambda: emit(null_rule=True),
        "emit: n_classes 0": lambda: emit(rule=_rule(n_classes=0)), "emit: n_classes 33": lambda: emit(rule=_rule(n_classes=33)),
        "emit: proj_size 0": lambda: emit(rule=_rule(proj_size=0.0)), "emit: proj_size nan": lambda: emit(rule=_rule(proj_size=float("nan"))),
        "emit: rows_per_batch does not divide": lambda: emit(per=48), "emit: rows_per_batch 0": lambda: emit(per=0),
        "emit: negative n_instances": lambda: emit(groups=1, n_ins=-1, group=out, ids=out),
        "emit: n_instances above n_rows": lambda: emit(groups=1, n_ins=65, group=out, ids=out),
        "emit: n_instances above 32768": lambda: emit(n=65536, per=65536, groups=1, n_ins=32769, group=out, ids=out),
        "emit: null group_instances": lambda: emit(groups=1, n_ins=3, group=out),
        "emit: misaligned proj_tlp": lambda: emit(tlp=out + 2),
        "emit: misaligned classes": lambda: emit(outs=(out + 2, out, out, out, out)),
        "emit: misaligned scales3": lambda: emit(outs=(out, out + 1, out, out, out)),
        "emit: misaligned onehots": lambda: emit(outs=(out, out, out + 2, out, out)),
        "emit: misaligned proj_uv": lambda: emit(outs=(out, out, out, out + 2, out)),
        "emit: misaligned batch": lambda: emit(outs=(out, out, out, out, out + 4)),
        "emit: misaligned group": lambda: emit(groups=1, n_ins=3, group=out + 2, ids=out),
        "emit: misaligned group_instances": lambda: emit(groups=1, n_ins=3, group=out, ids=out + 1),
    }
    for what, call in bad_calls.items():
        assert call() == -1, what                               # GCV_ERR_INVALID_ARGUMENT, never GCV_ERR_HIP
        assert L.gcv_last_error().startswith(b"gcv_train_inputs_"), (what, L.gcv_last_error())
    assert list(counts) == [-7, -7]
    assert emit(n=0, per=0) == 0 and emit(n=0, per=5, p=None) == 0       # no rows: nothing to queue


def test_install_and_uninstall_restore_the_function():
    calls = []

    def original(instances, z_dim):
        calls.append((instances, z_dim))
        return "original"

    helpers = types.SimpleNamespace(get_z=original)
    T.install(helpers)
    installed = helpers.get_z
    assert installed is not original
    T.install(helpers)                                           # twice is once
    assert helpers.get_z is installed
    cpu = torch.zeros(1, 4, 1)
    assert helpers.get_z(cpu, 8) == "original" and calls == [(cpu, 8)]     # a CPU tensor goes to the function bound before
    assert helpers.get_z(cpu, None) == "original" and len(calls) == 2
    T.uninstall(helpers)
    assert helpers.get_z is original and not [k for k in vars(helpers) if k != "get_z"]
    T.uninstall(helpers)
    assert helpers.get_z is original


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.prepare(torch.zeros(1, 4, 9), T.RULE_GOOGLE_EARTH())
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.get_z(torch.zeros(1, 4, 1), 8)
    assert T.get_z(torch.zeros(1, 4, 1), None) is None


def test_stats_have_the_two_counters():
    T.reset_stats()
    assert T.stats() == {"prepare_calls": 0, "get_z_calls": 0}
