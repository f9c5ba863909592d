"""numpy formulation of the pooling plan of gcs_pool_plan_* (include/gcs.h), written from its statement: the clusters of
`code[0] >> shift`, the rows by cluster with ties to the lower row, the head of each cluster and the pooled point set's
code, order and inverse.  Tests compare the library and the recorded reference run against it."""
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


def segments(idx_ptr, n):
    """cluster [n] for rows laid out by a hand-made idx_ptr over positions (row j of the sorted order is in the segment
    whose range holds j); -1 for a position in no segment."""
    out = np.full(n, -1, np.int64)
    for c in range(len(idx_ptr) - 1):
        out[idx_ptr[c]:idx_ptr[c + 1]] = c
    return out
