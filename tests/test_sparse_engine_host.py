"""The engines of libgcs_hip.so's convolution (include/gcs.h ABI v3), host side (not gpu; no device is
touched): the plan and workspace queries of both engines over a grid of shapes, the refusals of the `_engine` entry points
with their gcs_last_error texts, and the Python switch (set_engine / get_engine / GCS_ENGINE / stats)."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

from gaussiancity_amd import _native_s as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [1, 31, 32, 33, 73, 271, 1063, 4292, 16384, 32641, 262144]
CHANNELS = [(128, 32), (32, 32), (64, 64), (256, 256), (512, 512), (20, 24), (136, 200), (6, 5)]
KVOLS = [1, 15, 27, 125]
GRID = list(itertools.product(ROWS, CHANNELS, KVOLS))
TILE_ROWS_COLS = {S.TILE_32X32: (32, 32), S.TILE_64X64: (64, 64), S.TILE_128X32: (128, 32)}


def _workgroups(tile, n, nout):
    tm, tn = TILE_ROWS_COLS[tile]
    return -(-n // tm) * -(-nout // tn)


def _align(b):
    return (b + 255) // 256 * 256


def test_valu_engine_plan_is_the_plan():
    for n, (cin, cout), K in GRID:
        plan = S.subm_engine_plan(S.ENGINE_VALU, n, cin, cout, K)
        assert plan[:5] == S.subm_plan(n, cin, cout, K), (n, cin, cout, K)
        assert plan[5:] == (1, 1), (n, cin, cout, K)


def test_mfma_engine_plan_keeps_the_tiles_and_slices_only_small_grids():
    sliced = 0
    for n, (cin, cout), K in GRID:
        what = (n, cin, cout, K)
        plan = S.subm_engine_plan(S.ENGINE_MFMA, n, cin, cout, K)
        assert plan[:5] == S.subm_plan(n, cin, cout, K), what
        assert plan == S.subm_engine_plan(S.ENGINE_MFMA, n, cin, cout, K), what
        for tile, nout, slices in ((plan[0], cout, plan[5]), (plan[1], cin, plan[6])):
            assert 1 <= slices <= K, what
            per = -(-K // slices)
            assert (slices - 1) * per < K, "%r: an empty slice" % (what,)
            if _workgroups(tile, n, nout) >= 256:
                assert slices == 1, "%r: a grid that fills the GPU is sliced" % (what,)
            sliced += slices > 1
    assert sliced > 50
    for n, c in ((73, 512), (271, 256)):
        plan = S.subm_engine_plan(S.ENGINE_MFMA, n, c, c, 27)
        assert plan[5] > 1 and plan[6] > 1, (n, c, plan)


def test_workspace_sizes():
    L = S.lib()
    for (n, (cin, cout), K), dups in itertools.product(GRID, (0, 1)):
        what = (n, cin, cout, K, dups)
        old = L.gcs_subm_backward_workspace_bytes(n, cin, cout, K, dups)
        assert old > 0
        assert S.subm_engine_workspace_bytes(S.ENGINE_VALU, n, cin, cout, K, dups) == (0, old), what
        plan = S.subm_engine_plan(S.ENGINE_MFMA, n, cin, cout, K)
        fwd, bwd = S.subm_engine_workspace_bytes(S.ENGINE_MFMA, n, cin, cout, K, dups)
        if plan[5] == 1:
            assert fwd == 0, what
        else:
            assert fwd >= 4 * plan[5] * n * cout, what
        assert bwd >= old + (4 * plan[6] * n * cin if plan[6] > 1 else 0), what
        assert bwd <= old + _align(4 * plan[6] * n * cin), what       # and nothing else is added
    assert S.subm_engine_workspace_bytes(S.ENGINE_MFMA, 0, 8, 8, 27, 0)[0] == 0


def test_refusals_come_with_their_text_before_anything_is_queued():
    L = S.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    plan = (C.c_int32 * 7)()
    f, b = C.c_size_t(0), C.c_size_t(0)
    n, c, K = 73, 512, 27
    # engine 2
    assert L.gcs_subm_engine_plan(2, n, c, c, K, plan) == -1
    assert L.gcs_last_error() == b"gcs_subm_engine_plan: unknown engine (GCS_ENGINE_VALU or GCS_ENGINE_MFMA)"
    assert L.gcs_subm_engine_workspace_bytes(2, n, c, c, K, 0, C.byref(f), C.byref(b)) == -1
    assert b"gcs_subm_engine_workspace_bytes: unknown engine" in L.gcs_last_error()
    assert L.gcs_subm_forward_engine(2, p, n, K, p, c, p, None, c, p, p, 1 << 30, None) == -1
    assert b"gcs_subm_forward_engine: unknown engine" in L.gcs_last_error()
    assert L.gcs_subm_backward_engine(-1, p, n, K, 0, p, c, p, c, p, p, p, p, p, 1 << 30, None) == -1
    assert b"gcs_subm_backward_engine: unknown engine" in L.gcs_last_error()
    with pytest.raises(RuntimeError, match="unknown engine"):
        S.subm_engine_plan(2, n, c, c, K)
    # a null plan, null outputs of the size query, sizes out of range
    assert L.gcs_subm_engine_plan(S.ENGINE_MFMA, n, c, c, K, None) == -1
    assert L.gcs_last_error() == b"gcs_subm_engine_plan: null plan"
    assert L.gcs_subm_engine_workspace_bytes(S.ENGINE_MFMA, n, c, c, K, 0, None, C.byref(b)) == -1
    assert L.gcs_last_error() == b"gcs_subm_engine_workspace_bytes: null output"
    assert L.gcs_subm_engine_plan(S.ENGINE_MFMA, n, 0, c, K, plan) == -1
    assert b"channel count out of range" in L.gcs_last_error()
    # a sliced forward without its workspace, and with one a byte too small
    fwd, bwd = S.subm_engine_workspace_bytes(S.ENGINE_MFMA, n, c, c, K, 0)
    assert S.subm_engine_plan(S.ENGINE_MFMA, n, c, c, K)[5] > 1 and fwd > 0
    text = b"gcs_subm_forward_engine: workspace missing or smaller than gcs_subm_engine_workspace_bytes"
    assert L.gcs_subm_forward_engine(S.ENGINE_MFMA, p, n, K, p, c, p, None, c, p, None, fwd, None) == -1
    assert L.gcs_last_error() == text
    assert L.gcs_subm_forward_engine(S.ENGINE_MFMA, p, n, K, p, c, p, None, c, p, p, fwd - 1, None) == -1
    assert L.gcs_last_error() == text
    # the backward: the sliced dX's share of the workspace is asked for
    old = L.gcs_subm_backward_workspace_bytes(n, c, c, K, 0)
    assert bwd > old
    assert L.gcs_subm_backward_engine(S.ENGINE_MFMA, p, n, K, 0, p, c, p, c, p, p, p, p, p, old, None) == -1
    assert L.gcs_last_error() == b"gcs_subm_backward_engine: workspace missing or smaller than gcs_subm_engine_workspace_bytes"
    assert L.gcs_subm_backward_engine(S.ENGINE_VALU, p, n, K, 0, p, c, p, c, p, p, p, p, p, old - 1, None) == -1
    assert L.gcs_last_error() == b"gcs_subm_backward_engine: workspace missing or smaller than gcs_subm_backward_workspace_bytes"
    # n == 0 asks for nothing and queues nothing
    assert L.gcs_subm_forward_engine(S.ENGINE_MFMA, p, 0, K, None, c, p, None, c, None, None, 0, None) == 0


def test_set_engine_round_trip_and_bad_names():
    from gaussiancity_amd import sparse as SP
    first = SP.get_engine()
    try:
        assert SP.set_engine("mfma") == first and SP.get_engine() == "mfma"
        assert SP.set_engine("valu") == "mfma" and SP.get_engine() == "valu"
        for bad in ("MFMA", "", "vale", None, 1):
            with pytest.raises(ValueError, match="valu.*mfma"):
                SP.set_engine(bad)
            assert SP.get_engine() == "valu"
    finally:
        SP.set_engine(first)


def _child(env_value, code):
    env = dict(os.environ)
    env.pop("GCS_ENGINE", None)
    if env_value is not None:
        env["GCS_ENGINE"] = env_value
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)


def test_gcs_engine_environment_variable_in_a_fresh_process():
    code = "from gaussiancity_amd import sparse; print(sparse.get_engine())"
    r = _child(None, code)
    assert r.returncode == 0 and r.stdout.strip() == "valu", r.stderr
    r = _child("mfma", code)
    assert r.returncode == 0 and r.stdout.strip() == "mfma", r.stderr
    r = _child("tensor", code)
    assert r.returncode != 0 and "ValueError" in r.stderr and "valu" in r.stderr and "mfma" in r.stderr


def test_stats_count_forwards_per_engine_and_reset():
    from gaussiancity_amd import sparse as SP
    keys = ("conv_forward_calls_valu", "conv_forward_calls_mfma")
    assert all(k in SP.stats() for k in keys)
    SP._STATS["conv_forward_calls_mfma"] += 3
    SP._STATS["conv_forward_calls_valu"] += 2
    assert SP.stats()["conv_forward_calls_mfma"] >= 3
    SP.reset_stats()
    assert all(SP.stats()[k] == 0 for k in keys) and SP.stats()["rulebook_builds"] == 0
