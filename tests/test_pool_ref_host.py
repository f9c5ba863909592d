"""The reference formulations of tests/pool_ref.py and the case builders of tests/pool_cases.py, held to what they promise
without a GPU: plan_fast is plan(); gather_reduce, gather_backward and expand_add are the contract of include/gcs.h
written as plain Python loops, to the bit; and every case of tests/test_pool_frame_gpu.py is as large as the path it is
meant to reach (gaussiancity_amd/csrc/gcs_pool.h).

No input holds a NaN: the contract words min and max as comparisons, and a NaN's place in them is not part of it."""
import os
import re

import numpy as np
import pytest

import pool_cases as K
import pool_ref as R
from test_point_pool_gpu import _codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCES = ("sum", "mean", "min", "max")
DTYPES = (np.float32, np.float16)
# Read from the named constants on top of pool_cases.py, which name GP_MAX_BLOCKS and GP_THREADS of
# gaussiancity_amd/csrc/gcs_pool.h and IX_TILE and IX_SCAN_MIN_BLOCKS of gaussiancity_amd/csrc/gcs_index.h;
# test_case_constants_are_the_headers compares them with the headers' text.
GRID_CAP = K.GP_MAX_BLOCKS * K.GP_THREADS
IX_TILE = K.IX_TILE
IX_SCAN_MIN_BLOCKS = K.IX_SCAN_MIN_BLOCKS


def _bits(a):
    return a.view({4: np.uint32, 2: np.uint16, 8: np.uint64}[a.dtype.itemsize])


def test_case_constants_are_the_headers():
    """A change of a constant in the headers fails here, instead of silently moving a case off the path it was built for."""
    csrc = os.path.join(ROOT, "gaussiancity_amd", "csrc")
    text = open(os.path.join(csrc, "gcs_pool.h")).read() + open(os.path.join(csrc, "gcs_index.h")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, name
        return int(m.group(1))

    for name in ("GP_THREADS", "GP_MAX_BLOCKS", "IX_THREADS", "IX_ITEMS", "IX_SCAN_MIN_BLOCKS"):
        assert const(name) == getattr(K, name), name
    assert re.search(r"constexpr\s+int\s+IX_TILE\s*=\s*IX_THREADS\s*\*\s*IX_ITEMS\s*;", text)
    assert K.IX_TILE == K.IX_THREADS * K.IX_ITEMS == 4096 and GRID_CAP == K.GRID_CAP == 524288
    assert re.search(r"scanned\s*=\s*lay\.nb\s*>\s*IX_SCAN_MIN_BLOCKS", text)   # the path switch the large plans are about
    assert re.search(r"base\s*\+=\s*IX_THREADS", text)                          # k_pool_total's round


# ---------------------------------------------------------------------------------------------- plan_fast
def _same_plan(a, b):
    assert a._fields == b._fields == ("cluster", "indices", "idx_ptr", "head", "code", "order", "inverse", "n", "s")
    assert (a.n, a.s) == (b.n, b.s)
    for name in a._fields[:7]:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype == np.int64 and x.shape == y.shape and np.array_equal(x, y), name


@pytest.mark.parametrize("shift", [0, 3, 9])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 12293])
def test_plan_fast_is_plan(n, k, shift):
    rng = np.random.default_rng(1000 * n + 10 * k + shift)
    for pattern in ("mixed", "one", "distinct", "batch"):
        code = _codes(rng, pattern, n, k, shift)
        _same_plan(R.plan_fast(code, shift), R.plan(code, shift))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_plan_fast_is_plan_on_the_recorded_codes(case):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "ptv3_pool.npz"))
    code = golden["%s.int.in.serialized_code" % case]
    shift = 3 * {"a": 1, "b": 1, "c": 0}[case]
    _same_plan(R.plan_fast(code, shift), R.plan(code, shift))
    assert np.array_equal(R.plan_fast(code, shift).cluster, golden["%s.int.pooling_inverse" % case])


# ---------------------------------------------------------------------------------------------- the gathered reduce
def _loops(src, indices, idx_ptr, reduce):
    """The contract, one element at a time."""
    s, f, T = len(idx_ptr) - 1, src.shape[1], src.dtype.type
    out, arg = np.zeros((s, f), src.dtype), np.full((s, f), -1, np.int64)
    for c in range(s):
        lo, hi = int(idx_ptr[c]), int(idx_ptr[c + 1])
        for e in range(f):
            acc, res, best = np.float32(0), T(0), -1
            for j in range(lo, hi):
                r = int(indices[j])
                x = src[r, e]
                if reduce in ("sum", "mean"):
                    acc = np.float32(acc + np.float32(x))
                elif best < 0 or (np.float32(x) > np.float32(res) if reduce == "max" else np.float32(x) < np.float32(res)):
                    res, best = x, r
            if reduce == "mean" and hi > lo:
                acc = np.float32(acc / np.float32(hi - lo))
            out[c, e] = T(acc) if reduce in ("sum", "mean") else res
            arg[c, e] = best
    return out, (None if reduce in ("sum", "mean") else arg)


def _small_plan(seed):
    return K.hand_plan([3, 0, 1, 7, 2, 0, 65, 1, 8, 2, 40, 0], seed)   # 129 rows


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_reduce_is_the_contract_in_loops(dtype, ties):
    plan = _small_plan(1)
    src = K.values((plan.n, 5), dtype, 7, ties)
    for reduce in REDUCES:
        out, arg = R.gather_reduce(src, plan.indices, plan.idx_ptr, reduce)
        want, want_arg = _loops(src, plan.indices, plan.idx_ptr, reduce)
        assert out.dtype == dtype and np.array_equal(_bits(out), _bits(want)), reduce
        assert (arg is None and want_arg is None) or np.array_equal(arg, want_arg), reduce
        empty = np.diff(plan.idx_ptr) == 0
        assert empty.sum() == 3 and not _bits(out[empty]).any() and (arg is None or (arg[empty] == -1).all())
    if ties:   # the ties are there, and a tie matters: some other row of the segment holds the same value
        _, arg = R.gather_reduce(src, plan.indices, plan.idx_ptr, "max")
        rows = plan.indices[plan.idx_ptr[6]:plan.idx_ptr[7]]
        assert all((src[rows, e] == src[arg[6, e], e]).sum() > 1 for e in range(5))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_and_mean_lie_within_the_bars_of_a_float64_sum(dtype):
    """The bound of test_point_pool_gpu._bars: 1e-5 * sum|terms| in float32, 2^-11 * sum|terms| + 2^-24 in float16."""
    plan = K.hand_plan([1, 2, 8, 0, 65, 300, 3, 1, 2], 2)
    src = K.values((plan.n, 6), dtype, 8, False)
    cnt = np.diff(plan.idx_ptr)
    for reduce in ("sum", "mean"):
        got, _ = R.gather_reduce(src, plan.indices, plan.idx_ptr, reduce)
        for c in range(plan.s):
            rows = src[plan.indices[plan.idx_ptr[c]:plan.idx_ptr[c + 1]]].astype(np.float64)
            want, mass = rows.sum(0), np.abs(rows).sum(0)
            if reduce == "mean":
                want, mass = want / max(cnt[c], 1), mass / max(cnt[c], 1)
            bar = 1e-5 * mass if dtype == np.float32 else 2.0 ** -11 * mass + 2.0 ** -24
            assert (np.abs(got[c].astype(np.float64) - want) <= bar).all(), (reduce, c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_arg_is_the_first_attaining_row(dtype):
    """A segment whose values are all equal, one that mixes -0.0 and +0.0 (equal in the comparison: the first position
    keeps the value, with its sign), and a maximum that comes twice."""
    idx_ptr = np.array([0, 4, 8, 12, 12], np.int64)
    indices = np.array([5, 2, 9, 0, 11, 3, 7, 1, 10, 4, 8, 6], np.int64)   # positions -> source rows, in no order
    src = np.zeros((12, 2), dtype)
    src[[5, 2, 9, 0]] = 2.5                                # all equal
    src[[11, 3, 7, 1], 0] = [-0.0, 0.0, -0.0, 0.0]         # zeros of both signs, -0.0 first ...
    src[[11, 3, 7, 1], 1] = [0.0, -0.0, 0.0, -0.0]         # ... and +0.0 first
    src[[10, 4, 8, 6], 0] = [1.0, 3.0, 3.0, -2.0]          # the maximum twice; the minimum is last
    src[[10, 4, 8, 6], 1] = [-1.0, -1.0, 4.0, 4.0]         # the minimum twice, then the maximum twice
    for reduce, third, third_arg in (("max", [3.0, 4.0], [4, 8]), ("min", [-2.0, -1.0], [6, 10])):
        out, arg = R.gather_reduce(src, indices, idx_ptr, reduce)
        assert arg[0].tolist() == [5, 5] and out[0].tolist() == [2.5, 2.5]
        assert arg[1].tolist() == [11, 11] and np.signbit(out[1]).tolist() == [True, False]
        assert arg[2].tolist() == third_arg and out[2].tolist() == third
        assert arg[3].tolist() == [-1, -1] and not _bits(out[3]).any()
        want, want_arg = _loops(src, indices, idx_ptr, reduce)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(arg, want_arg)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_and_expand_add_are_the_transposes_in_loops(dtype):
    plan = _small_plan(3)
    f, T = 4, dtype
    src = K.values((plan.n, f), dtype, 9, True)
    dout = K.values((plan.s, f), dtype, 10, False)
    cnt = np.diff(plan.idx_ptr)
    for reduce in REDUCES:
        _, arg = R.gather_reduce(src, plan.indices, plan.idx_ptr, reduce)
        got = R.gather_backward(dout, plan.cluster, plan.idx_ptr, reduce, arg)
        want = np.zeros((plan.n, f), dtype)
        for r in range(plan.n):
            c = plan.cluster[r]
            for e in range(f):
                if reduce == "sum":
                    want[r, e] = dout[c, e]
                elif reduce == "mean":
                    want[r, e] = T(np.float32(dout[c, e]) / np.float32(cnt[c]))
                elif arg[c, e] == r:
                    want[r, e] = dout[c, e]
        assert got.dtype == dtype and np.array_equal(_bits(got), _bits(want)), reduce
        if reduce in ("min", "max"):   # one row of every non-empty segment has the gradient, per column
            assert ((got != 0).sum(0) <= (cnt > 0).sum()).all()
    a, b = K.values((plan.n, f), dtype, 11, False), K.values((plan.s, f), dtype, 12, False)
    got = R.expand_add(a, b, plan.cluster)
    want = np.array([[T(np.float32(a[r, e]) + np.float32(b[plan.cluster[r], e])) for e in range(f)] for r in range(plan.n)], dtype)
    assert got.dtype == dtype and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(R.expand_add(None, b, plan.cluster)), _bits(b[plan.cluster]))


# ---------------------------------------------------------------------------------------------- the cases' promises
def test_plan_sizes_have_more_than_two_tiles_and_more_than_256():
    for n in K.PLAN_TILE_SIZES + (K.N_PLACED,):
        assert 3 <= -(-n // IX_TILE) <= IX_SCAN_MIN_BLOCKS, n
    assert {n % IX_TILE for n in K.PLAN_TILE_SIZES} == {IX_TILE - 1, 0, 5, 17}
    tiles = -(-K.N_ROUNDS // IX_TILE)
    assert tiles == 257 and tiles > IX_SCAN_MIN_BLOCKS and tiles > K.IX_THREADS   # the scanned sort, k_pool_total's second round
    assert [c[0] for c in K.ROUNDS_CASES] == ["mixed", "one", "distinct"]
    pattern, k, shift = K.ROUNDS_CASES[2]
    # every key its own cluster: s = n, so the sort of the pooled rows (k - 1 of them) takes the scanned path as well
    assert k >= 2 and shift == 0 and -(-K.N_ROUNDS // IX_TILE) > IX_SCAN_MIN_BLOCKS


@pytest.mark.parametrize("name", list(K.placed_cases()))
@pytest.mark.parametrize("k,shift", [(1, 0), (3, 3)])
def test_placed_codes_put_the_heads_where_they_say(name, k, shift):
    n, heads = K.placed_cases()[name]
    sizes = K.sizes_for_heads(n, heads)
    code = K.placed_codes(sizes, k, shift, seed=5)
    assert code.shape == (k, n) and (code[0] < 0).any()
    assert sizes.size == 1 or not np.array_equal(code[0], np.sort(code[0]))   # the rows are shuffled
    plan = R.plan_fast(code, shift)
    want = sorted(set([0] + list(heads)))
    assert plan.s == len(want) and plan.idx_ptr[:-1].tolist() == want and plan.idx_ptr[-1] == n
    assert np.array_equal(np.diff(plan.idx_ptr), sizes)


def test_placed_cases_reach_the_edges_they_name():
    cases = K.placed_cases()
    T = IX_TILE
    assert set(cases["tile_edges"][1]) == {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1}
    n, heads = cases["thread_edges"]
    assert {h % K.IX_ITEMS for h in heads} == {K.IX_ITEMS - 1, 0, 1} and max(heads) > 3 * T and len(heads) == 3 * (n // K.IX_ITEMS)
    n, heads = cases["empty_tiles"]
    per_tile = np.bincount(np.array(heads) // T, minlength=5)
    assert n == 5 * T + 17 and per_tile.tolist()[1:4] == [0, 0, T] and per_tile[0] > 0 and per_tile[4] > 0
    assert T - 1 in heads   # the cluster over the two empty tiles opens at the last position of tile 0
    assert cases["one_cluster"] == (K.N_PLACED, []) and cases["all_distinct"][1] == list(range(K.N_PLACED))


@pytest.mark.parametrize("name", list(K.GRID_CASES))
def test_grid_cases_take_the_stride_loop_more_than_twice(name):
    f, dtype, vector, reduces = K.GRID_CASES[name]
    plan = K.grid_plan(name)
    sizes = np.diff(plan.idx_ptr)
    assert sizes.max() == K.LONG and set(sizes.tolist()) == set(K.CYCLE) | {K.LONG} and plan.n == sizes.sum()
    v = 16 // np.dtype(dtype).itemsize
    per_row = f // v if vector else f
    fwd, bwd, add = K.item_counts(name, plan)
    assert (fwd, bwd, add) == (plan.s * per_row, plan.n * per_row, plan.n * per_row)
    for items in (fwd, bwd, add):
        assert items > 2 * GRID_CAP and items >= K.MIN_TRIPS * GRID_CAP, (name, items)
    assert fwd < 2.4 * GRID_CAP or not vector   # the smallest that does it
    # the long segment's items belong to the second trip
    assert GRID_CAP <= (plan.s // 2) * per_row < 2 * GRID_CAP
    if vector:   # the same plan one element at a time (a slice one element off): more items still
        assert all(i > 2 * GRID_CAP for i in K.item_counts(name, plan, vector=False))
        assert 9000 <= plan.s <= 19000 and f == 512 and set(reduces) == set(REDUCES)
    else:
        assert 400000 <= plan.s <= 405000 and reduces == (("mean", "max") if f == 3 else REDUCES)


def test_hand_plan_is_a_plan():
    plan = K.grid_plan("wide_f32")
    assert np.array_equal(np.sort(plan.indices), np.arange(plan.n)) and np.array_equal(plan.cluster, K.reference_plan(plan))
    assert plan.idx_ptr[0] == 0 and plan.idx_ptr[-1] == plan.n and plan.idx_ptr.size == plan.s + 1
    x = K.values((1000, 8), np.float16, 1, True)
    assert np.isfinite(x).all() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
