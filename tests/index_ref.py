"""numpy formulation of the point backbone's index plans (include/gcs.h, gcs_serialize / gcs_patch_plan_*), written from
the definitions: the z interleave bit by bit, Skilling's axes-to-transpose for the Hilbert curve, the `cord` expression in
np.float32, a stable argsort, and the closed form of the padding plan.  tests/golden/ptv3_index.npz pins it to what
models/pt_v3.py computes on the CPU."""
import numpy as np

ORDERS = ("cord", "z", "z-trans", "hilbert", "hilbert-trans")


def _interleave(x, y, z, depth):
    """bit i of x, y, z -> bit 3i+2, 3i+1, 3i"""
    key = np.zeros(x.shape, np.int64)
    for i in range(depth):
        key |= ((x >> i) & 1) << (3 * i + 2) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i)
    return key


def _hilbert(x, y, z, depth):
    """Skilling, "Programming the Hilbert curve" (2004): axes to transpose, Gray step, interleave (axis 0 on top)."""
    X = [x.copy(), y.copy(), z.copy()]
    Q = 1 << (depth - 1)
    while Q > 1:
        P = Q - 1
        for i in range(3):
            on = (X[i] & Q) != 0
            t = np.where(on, 0, (X[0] ^ X[i]) & P)
            X[0] = np.where(on, X[0] ^ P, X[0] ^ t)
            if i:
                X[i] = X[i] ^ t
        Q >>= 1
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = 1 << (depth - 1)
    while Q > 1:
        t = np.where((X[2] & Q) != 0, t ^ (Q - 1), t)
        Q >>= 1
    return _interleave(X[0] ^ t, X[1] ^ t, X[2] ^ t, depth)


def codes(grid_coord, batch, depth, orders, grid_size=0.01):
    """int64 [len(orders), n]: the serialization codes.  grid_coord int [n, 3], batch int [n] or None."""
    g = np.asarray(grid_coord).astype(np.int64).reshape(-1, 3)
    m = (1 << depth) - 1
    x, y, z = g[:, 0] & m, g[:, 1] & m, g[:, 2] & m
    rows = []
    for name in orders:
        if name == "cord":
            f = g.astype(np.float32)
            c = (f[:, 0] / np.float32(grid_size ** 2) + f[:, 1] / np.float32(grid_size)) + f[:, 2]
            assert c.dtype == np.float32
            c = np.trunc(c).astype(np.int64)
        elif name == "z":
            c = _interleave(x, y, z, depth)
        elif name == "z-trans":
            c = _interleave(y, x, z, depth)
        elif name == "hilbert":
            c = _hilbert(x, y, z, depth)
        elif name == "hilbert-trans":
            c = _hilbert(y, x, z, depth)
        else:
            raise ValueError(name)
        if batch is not None:
            c = np.asarray(batch).astype(np.int64) << (3 * depth) | c
        rows.append(c)
    return np.stack(rows)


def order_inverse(code):
    """Signed ascending, ties to the lower row; inverse[r, order[r, j]] = j."""
    order = np.argsort(code, axis=1, kind="stable").astype(np.int64)
    inverse = np.empty_like(order)
    for r in range(order.shape[0]):
        inverse[r, order[r]] = np.arange(order.shape[1])
    return order, inverse


def serialize(grid_coord, batch, depth, orders, grid_size=0.01):
    code = codes(grid_coord, batch, depth, orders, grid_size)
    return (code,) + order_inverse(code)


def patch_plan(offset, patch_size):
    """(pad int64 [padded], unpad int64 [offset[-1]], cu_seqlens int32) from the inclusive row ends of the batches."""
    off = np.concatenate([[0], np.asarray(offset, np.int64)])
    P = int(patch_size)
    n = np.diff(off)
    n_pad = np.where(n > P, (n + P - 1) // P * P, n)
    off_pad = np.concatenate([[0], np.cumsum(n_pad)])
    pad = np.empty(int(off_pad[-1]), np.int64)
    unpad = np.empty(int(off[-1]), np.int64)
    cu = []
    for i in range(len(n)):
        s = off_pad[i] - off[i]
        unpad[off[i]:off[i + 1]] = np.arange(off[i], off[i + 1]) + s
        p = np.arange(off_pad[i], off_pad[i + 1])
        pad[off_pad[i]:off_pad[i + 1]] = np.where(p >= off_pad[i] + n[i], p - P, p) - s
        cu.extend(range(int(off_pad[i]), int(off_pad[i + 1]), P))
    cu.append(int(off_pad[-1]))
    return pad, unpad, np.asarray(cu, np.int32)
