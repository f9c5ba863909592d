"""numpy formulation of the pooling plan of gcs_pool_plan_* (include/gcs.h), written from its statement: the clusters of
`code[0] >> shift`, the rows by cluster with ties to the lower row, the head of each cluster and the pooled point set's
code, order and inverse.  Tests compare the library and the recorded reference run against it.  plan_fast is the same plan
without a loop over rows; gather_reduce, gather_backward and expand_add are the gathered reduce of gcs_segment_gather_*
and gcs_segment_expand_add_t to the bit.  numpy only: nothing here calls the library."""
import collections

import numpy as np

Plan = collections.namedtuple("Plan", "cluster indices idx_ptr head code order inverse n s")


def order_inverse(code):
    """order[r] sorts code[r] ascending as signed int64, ties to the lower position; inverse[r][order[r][c]] = c."""
    code = np.asarray(code, np.int64)
    order = np.stack([np.argsort(row, kind="stable") for row in code]).astype(np.int64)
    inverse = np.empty_like(order)
    for r in range(code.shape[0]):
        inverse[r, order[r]] = np.arange(code.shape[1], dtype=np.int64)
    return order, inverse


def plan(code, shift):
    """The plan for code int64 [k, n] and shift = 3 * pooling_depth."""
    code = np.asarray(code, np.int64)
    assert code.ndim == 2 and code.shape[1] >= 1 and 0 <= shift <= 48 and shift % 3 == 0
    k, n = code.shape
    key = code[0] >> shift  # numpy shifts a signed integer arithmetically
    distinct = sorted(set(key.tolist()))
    number = {v: c for c, v in enumerate(distinct)}
    cluster = np.array([number[v] for v in key.tolist()], np.int64)
    s = len(distinct)
    sizes = np.zeros(s, np.int64)
    for c in cluster:
        sizes[c] += 1
    idx_ptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(sizes)]).astype(np.int64)
    indices = np.array(sorted(range(n), key=lambda j: (cluster[j], j)), np.int64)
    head = indices[idx_ptr[:-1]]
    down = code[:, head] >> shift
    order, inverse = order_inverse(down)
    return Plan(cluster, indices, idx_ptr, head, down, order, inverse, n, s)


def plan_fast(code, shift):
    """plan() once more without a Python loop over rows, for point sets of a million rows: a stable argsort of the keys,
    a head flag where the sorted key changes, its running sum as the cluster number.  tests/test_pool_ref_host.py pins it
    to plan(), which stays the formulation from the statement."""
    code = np.asarray(code, np.int64)
    assert code.ndim == 2 and code.shape[1] >= 1 and 0 <= shift <= 48 and shift % 3 == 0
    n = code.shape[1]
    key = code[0] >> shift
    indices = np.argsort(key, kind="stable").astype(np.int64)
    ordered = key[indices]
    flag = np.ones(n, bool)
    flag[1:] = ordered[1:] != ordered[:-1]
    starts = np.flatnonzero(flag).astype(np.int64)
    s = int(starts.size)
    cluster = np.empty(n, np.int64)
    cluster[indices] = np.cumsum(flag, dtype=np.int64) - 1
    idx_ptr = np.concatenate([starts, np.array([n], np.int64)])
    head = indices[starts]
    down = code[:, head] >> shift
    order = np.argsort(down, axis=1, kind="stable").astype(np.int64)
    inverse = np.empty_like(order)
    np.put_along_axis(inverse, order, np.broadcast_to(np.arange(s, dtype=np.int64), order.shape), axis=1)
    return Plan(cluster, indices, idx_ptr, head, down, order, inverse, n, s)


# ---- the gathered reduce of gcs_segment_gather_* and gcs_segment_expand_add_t, to the bit (include/gcs.h): every step is
# one IEEE operation in numpy's float32, so what comes out is what the contract prescribes, not an approximation of it.
# Inputs are float32 or float16 arrays without NaN (a comparison with NaN is outside the contract's wording).
def _counts(idx_ptr):
    return np.diff(np.asarray(idx_ptr, np.int64))


def gather_reduce(src, indices, idx_ptr, reduce):
    """(out [s, f], arg int64 [s, f] or None) of `reduce` over src[indices[j]], j in [idx_ptr[c], idx_ptr[c + 1]).
    sum, mean: one float32 chain from 0 in ascending j; mean divides by float32(count) where the count is not 0; one
    conversion to src's dtype (round to nearest even).  min, max: strict comparison in float32, the bits of the attaining
    element copied, arg the SOURCE row of the first j that attains the value.  An empty segment gives 0 and -1.
    Vectorised over the segments, a loop over the position within the segment."""
    assert reduce in ("sum", "mean", "min", "max") and src.ndim == 2 and src.dtype in (np.float32, np.float16)
    indices, idx_ptr, count = np.asarray(indices, np.int64), np.asarray(idx_ptr, np.int64), _counts(idx_ptr)
    s, f = count.size, src.shape[1]
    by_size = np.argsort(-count, kind="stable")   # segments with more than t rows are by_size[:live]
    alive = np.searchsorted(-count[by_size], -np.arange(int(count.max(initial=0))), side="left")
    if reduce in ("sum", "mean"):
        acc = np.zeros((s, f), np.float32)
        for t, live in enumerate(alive):
            seg = by_size[:live]
            acc[seg] = acc[seg] + src[indices[idx_ptr[seg] + t]].astype(np.float32)
        if reduce == "mean":
            full = count > 0
            acc[full] = acc[full] / count[full].astype(np.float32)[:, None]
        return acc.astype(src.dtype), None
    res, arg = np.zeros((s, f), src.dtype), np.full((s, f), -1, np.int64)
    for t, live in enumerate(alive):
        seg = by_size[:live]
        rows = indices[idx_ptr[seg] + t]
        x, cur = src[rows], res[seg]
        x32, cur32 = x.astype(np.float32), cur.astype(np.float32)
        better = (arg[seg] < 0) | (x32 > cur32 if reduce == "max" else x32 < cur32)
        res[seg] = np.where(better, x, cur)
        arg[seg] = np.where(better, rows[:, None], arg[seg])
    return res, arg


def gather_backward(dout, cluster, idx_ptr, reduce, arg=None):
    """dsrc [n, f], the transpose by row: dout[cluster[r]] (sum), that divided by float32(count) in float32 and rounded
    once (mean), or that where arg[cluster[r]] == r and 0 elsewhere (min, max).  Every row is in a segment."""
    cluster, count = np.asarray(cluster, np.int64), _counts(idx_ptr)
    g = dout[cluster]
    if reduce == "sum":
        return g
    if reduce == "mean":
        return (g.astype(np.float32) / count[cluster].astype(np.float32)[:, None]).astype(dout.dtype)
    rows = np.arange(cluster.size, dtype=np.int64)[:, None]
    return np.where(arg[cluster] == rows, g, np.zeros((), dout.dtype))


def expand_add(a, b, cluster):
    """a[r] + b[cluster[r]]: one float32 add, rounded once to the dtype; without a, b's bits."""
    g = b[np.asarray(cluster, np.int64)]
    return g if a is None else (a.astype(np.float32) + g.astype(np.float32)).astype(b.dtype)


def segments(idx_ptr, n):
    """cluster [n] for rows laid out by a hand-made idx_ptr over positions (row j of the sorted order is in the segment
    whose range holds j); -1 for a position in no segment."""
    out = np.full(n, -1, np.int64)
    for c in range(len(idx_ptr) - 1):
        out[idx_ptr[c]:idx_ptr[c + 1]] = c
    return out
