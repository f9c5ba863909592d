"""The cases of tests/test_pool_frame_gpu.py, in numpy and without a GPU, so that tests/test_pool_ref_host.py can hold them
to what they promise: plans whose heads sit at chosen sorted positions, and hand-made plans whose gathered reduce has
more work items than one grid of the kernels covers (gaussiancity_amd/csrc/gcs_pool.h)."""
import collections

import numpy as np

import pool_ref as R

# The constants of the kernels that decide which path a size takes.  tests/test_pool_ref_host.py reads the headers and
# fails when one of them moves: GP_THREADS and GP_MAX_BLOCKS in gaussiancity_amd/csrc/gcs_pool.h; IX_THREADS, IX_ITEMS,
# IX_TILE (= IX_THREADS * IX_ITEMS) and IX_SCAN_MIN_BLOCKS in gaussiancity_amd/csrc/gcs_index.h.
GP_THREADS = 256
GP_MAX_BLOCKS = 2048
IX_THREADS = 256
IX_ITEMS = 16
IX_TILE = IX_THREADS * IX_ITEMS
IX_SCAN_MIN_BLOCKS = 256
GRID_CAP = GP_MAX_BLOCKS * GP_THREADS   # threads of the largest grid: an item count beyond it is a second trip of the loop
PIECE_BYTES = 16

# ---------------------------------------------------------------------------------------------- plans
PLAN_TILE_SIZES = (3 * IX_TILE - 1, 3 * IX_TILE, 3 * IX_TILE + 5, 5 * IX_TILE + 17)
N_PLACED = 3 * IX_TILE + 5
N_ROUNDS = IX_SCAN_MIN_BLOCKS * IX_TILE + 1   # 257 tiles: k_pool_total's second round, the sort's scan kernel
ROUNDS_CASES = (("mixed", 2, 3), ("one", 1, 0), ("distinct", 2, 0))   # (pattern of _codes, k, shift)


def sizes_for_heads(n, heads):
    """Cluster sizes for which the sorted positions of the heads are exactly `heads` (position 0 is always one)."""
    starts = np.unique(np.concatenate([[0], np.asarray(heads, np.int64)]))
    assert starts[0] == 0 and starts[-1] < n
    return np.diff(np.concatenate([starts, [n]])).astype(np.int64)


def placed_codes(sizes, k=1, shift=0, negative=3, seed=0):
    """code int64 [k, n] whose cluster c has sizes[c] rows and the key c - negative (so the first `negative` keys are
    below zero), rows shuffled: the heads are at the sorted positions cumsum(sizes) - sizes.  Below the shift, and in the
    other order rows, the bits are drawn at random (eight values after the shift: down_code is full of ties)."""
    sizes = np.asarray(sizes, np.int64)
    assert sizes.min() >= 1
    rng = np.random.default_rng(seed)
    n = int(sizes.sum())
    key = np.repeat(np.arange(sizes.size, dtype=np.int64) - negative, sizes)
    row0 = (key << shift | rng.integers(0, 1 << shift, n))[rng.permutation(n)]
    rows = [row0] + [rng.integers(0, 8, n) << shift | rng.integers(0, 1 << shift, n) for _ in range(k - 1)]
    return np.stack(rows).astype(np.int64)


def placed_cases():
    """name -> (n, head positions) of the plans with cluster sizes placed on purpose."""
    n, T = N_PLACED, IX_TILE
    cases = collections.OrderedDict()
    cases["tile_edges"] = (n, [T * t + d for t in (1, 2, 3) for d in (-1, 0, 1)])
    cases["thread_edges"] = (n, [IX_ITEMS * j + d for j in range(1, n // IX_ITEMS + 1) for d in (-1, 0, 1) if IX_ITEMS * j + d < n])
    # tile 0: a head every third position, the last one at T - 1; its cluster covers tiles 1 and 2 entirely, which so have
    # no head; tile 3 is single-row clusters throughout; tile 4 is clusters of two
    m = 5 * T + 17
    cases["empty_tiles"] = (m, list(range(0, T, 3)) + list(range(3 * T, 4 * T)) + list(range(4 * T, m, 2)))
    cases["one_cluster"] = (n, [])
    cases["all_distinct"] = (n, list(range(n)))
    return cases


# ---------------------------------------------------------------------------------------------- gathered reduce
HandPlan = collections.namedtuple("HandPlan", "cluster indices idx_ptr head n s")
CYCLE = (1, 2, 0, 3, 8)
LONG = 300
MIN_TRIPS = 2.3   # two whole trips of the grid-stride loop and part of a third


def pieces(f, dtype, vector):
    """Work items per row: 16-byte pieces, or single elements."""
    v = PIECE_BYTES // np.dtype(dtype).itemsize
    assert not vector or f % v == 0
    return f // v if vector else f


def cycle_sizes(s):
    """s segment sizes cycling through CYCLE, the one in the middle LONG rows."""
    sizes = np.array([CYCLE[i % len(CYCLE)] for i in range(s)], np.int64)
    sizes[s // 2] = LONG
    return sizes


def hand_plan(sizes, seed):
    """A plan with these segment sizes over a random permutation of the rows; the head of an empty segment is a row of
    its neighbour, which nothing reads."""
    sizes = np.asarray(sizes, np.int64)
    m = int(sizes.sum())
    idx_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    indices = np.random.default_rng(seed).permutation(m).astype(np.int64)
    cluster = np.empty(m, np.int64)
    cluster[indices] = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    head = indices[np.minimum(idx_ptr[:-1], m - 1)]
    return HandPlan(cluster, indices, idx_ptr, head, m, int(sizes.size))


def segments_for(f, dtype, vector):
    """The fewest segments, rounded up to a hundred, whose forward items reach MIN_TRIPS grids."""
    need = int(np.ceil(MIN_TRIPS * GRID_CAP / pieces(f, dtype, vector)))
    return -(-need // 100) * 100


# name -> (f, dtype, 16-byte pieces?, reduces).  Forward items are s * pieces, backward and expand-add items n * pieces.
# "wide" has 9 500 segments in float32 and 18 900 in float16, whose pieces hold twice the elements.
GRID_CASES = collections.OrderedDict([
    ("wide_f32", (512, "float32", True, ("sum", "mean", "min", "max"))),
    ("wide_f16", (512, "float16", True, ("sum", "mean", "min", "max"))),
    ("coord_f32", (3, "float32", False, ("mean", "max"))),
    ("coord_f16", (3, "float16", False, ("mean", "max"))),
    ("five_f32", (5, "float32", False, ("sum", "mean", "min", "max"))),
    ("five_f16", (5, "float16", False, ("sum", "mean", "min", "max"))),
])


def grid_plan(name):
    """The case's plan.  The one-element cases share the segment count of f = 3 (402 000)."""
    f, dtype, vector, _ = GRID_CASES[name]
    s = segments_for(f, dtype, True) if vector else segments_for(3, dtype, False)
    return hand_plan(cycle_sizes(s), sorted(GRID_CASES).index(name))


def item_counts(name, plan=None, vector=None):
    """(forward, backward, expand-add) work items of a case."""
    f, dtype, vec, _ = GRID_CASES[name]
    plan = grid_plan(name) if plan is None else plan
    p = pieces(f, dtype, vec if vector is None else vector)
    return plan.s * p, plan.n * p, plan.n * p


def values(shape, dtype, seed, ties):
    """Finite values without NaN: normal deviates, or the integers -3...3 (full of ties; -0.0 among the zeros)."""
    rng = np.random.default_rng(seed)
    if not ties:
        return rng.standard_normal(shape).astype(dtype)
    x = rng.integers(-3, 4, shape).astype(dtype)
    x[(x == 0) & (rng.random(shape) < 0.5)] = -0.0
    return x


def reference_plan(plan):
    """R.segments is the statement; hand_plan's cluster must be it."""
    want = np.empty(plan.n, np.int64)
    want[plan.indices] = R.segments(plan.idx_ptr, plan.n)
    return want
