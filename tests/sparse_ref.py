"""Float64 numpy reference of the sparse operators (gaussiancity_amd.sparse), written from
the stated rules: packed voxel keys and np.searchsorted for neighbours, the lowest row of a voxel as its
representative, submanifold convolution forward / dX / dW / dB, segment_csr and its gradients.  Every result comes
with a scale (the sum of the absolute values of its terms) that sets the tolerance of a float32 comparison.

shell_cloud() makes seeded synthetic "building shell" clouds: voxelised faces of random hollow boxes."""
import numpy as np


def pack(indices, spatial_shape):
    b, a, c, d = (indices[:, q].astype(np.int64) for q in range(4))
    s0, s1, s2 = (int(s) for s in spatial_shape)
    return ((b * s0 + a) * s1 + c) * s2 + d


def tap_offsets(ksize, dilation):
    """[K, 3] offsets of the taps, tap k = (a * k1 + b) * k2 + c, centre = k // 2."""
    k0, k1, k2 = ksize
    a, b, c = np.meshgrid(np.arange(k0), np.arange(k1), np.arange(k2), indexing="ij")
    off = np.stack([(a - k0 // 2) * dilation[0], (b - k1 // 2) * dilation[1], (c - k2 // 2) * dilation[2]], -1)
    return off.reshape(-1, 3)


def neighbours(indices, spatial_shape, ksize, dilation):
    """nbr [N, K]: row index of the representative (lowest row) at coordinate + offset, or -1."""
    indices = np.asarray(indices, np.int64)
    n = len(indices)
    keys = pack(indices, spatial_shape)
    rows = np.arange(n)
    order = np.lexsort((rows, keys))
    uk, first = np.unique(keys[order], return_index=True)
    rep_of = order[first]                                  # lowest row of every distinct key
    off = tap_offsets(ksize, dilation)
    nbr = np.full((n, len(off)), -1, np.int64)
    shape = np.asarray(spatial_shape, np.int64)
    for k, o in enumerate(off):
        q = indices.copy()
        q[:, 1:] += o
        inside = np.all((q[:, 1:] >= 0) & (q[:, 1:] < shape), axis=1)
        if n == 0:
            continue
        kk = pack(q, spatial_shape)
        pos = np.clip(np.searchsorted(uk, kk), 0, max(len(uk) - 1, 0))
        found = inside & (uk[pos] == kk)
        nbr[found, k] = rep_of[pos[found]]
    return nbr


def _weights(w):
    """[Cout, kD, kH, kW, Cin] -> [Cout, K, Cin] float64."""
    w = np.asarray(w, np.float64)
    return w.reshape(w.shape[0], -1, w.shape[-1])


def conv_forward(x, w, bias, nbr):
    """y [N, Cout] and its scale."""
    x = np.asarray(x, np.float64)
    W = _weights(w)
    n, cout = x.shape[0], W.shape[0]
    y = np.zeros((n, cout))
    sc = np.zeros((n, cout))
    if bias is not None:
        y += np.asarray(bias, np.float64)
        sc += np.abs(np.asarray(bias, np.float64))
    for k in range(W.shape[1]):
        m = nbr[:, k] >= 0
        if not m.any():
            continue
        g = x[nbr[m, k]]
        y[m] += g @ W[:, k, :].T
        sc[m] += np.abs(g) @ np.abs(W[:, k, :]).T
    return y, sc


def conv_backward(x, w, nbr, dy):
    """(dx, dw, db) and their scales, straight from the definition: dx[j] += W_k^T dy[i] for every nbr[i, k] = j."""
    x = np.asarray(x, np.float64)
    dy = np.asarray(dy, np.float64)
    W = _weights(w)
    cout, K, cin = W.shape
    dx, sdx = np.zeros_like(x), np.zeros_like(x)
    dw, sdw = np.zeros((cout, K, cin)), np.zeros((cout, K, cin))
    for k in range(K):
        m = nbr[:, k] >= 0
        if not m.any():
            continue
        j = nbr[m, k]
        g = dy[m]
        if len(np.unique(j)) == len(j):          # distinct voxels: one row per target, a plain scatter
            dx[j] += g @ W[:, k, :]
            sdx[j] += np.abs(g) @ np.abs(W[:, k, :])
        else:
            np.add.at(dx, j, g @ W[:, k, :])
            np.add.at(sdx, j, np.abs(g) @ np.abs(W[:, k, :]))
        dw[:, k, :] = g.T @ x[j]
        sdw[:, k, :] = np.abs(g).T @ np.abs(x[j])
    shape = np.asarray(w).shape
    return (dx, sdx), (dw.reshape(shape), sdw.reshape(shape)), (dy.sum(0), np.abs(dy).sum(0))


def dense_conv_check(x, w, bias, indices, spatial_shape, batch_size, dilation):
    """The same convolution through torch.nn.functional.conv3d on the densified grid (float64); rows must be
    distinct voxels.  Pins the orientation of this reference."""
    import torch
    import torch.nn.functional as F
    idx = np.asarray(indices, np.int64)
    cin = x.shape[1]
    dense = torch.zeros((batch_size, cin) + tuple(spatial_shape), dtype=torch.float64)
    dense[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = torch.from_numpy(np.asarray(x, np.float64))
    wt = torch.from_numpy(np.asarray(w, np.float64)).permute(0, 4, 1, 2, 3)
    ks = wt.shape[2:]
    pad = tuple(d * (k // 2) for d, k in zip(dilation, ks))
    out = F.conv3d(dense, wt, None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)), padding=pad,
                   dilation=tuple(dilation))
    return out[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]].numpy()


def segment_csr(src, indptr, reduce):
    """(out, scale, arg) of torch_scatter.segment_csr along dim 0; arg (min / max) is the first row attaining
    the value, -1 for an empty segment."""
    src = np.asarray(src, np.float64)
    m = src.shape[0]
    flat = src.reshape(m, -1)
    s = len(indptr) - 1
    out = np.zeros((s, flat.shape[1]))
    sc = np.zeros_like(out)
    arg = np.full(out.shape, -1, np.int64)
    for q in range(s):
        lo, hi = int(indptr[q]), int(indptr[q + 1])
        if hi <= lo:
            continue
        seg = flat[lo:hi]
        if reduce in ("sum", "add", "mean"):
            out[q] = seg.sum(0)
            sc[q] = np.abs(seg).sum(0)
            if reduce == "mean":
                out[q] /= hi - lo
                sc[q] /= hi - lo
        else:
            a = seg.argmax(0) if reduce == "max" else seg.argmin(0)   # numpy: first index among ties
            arg[q] = lo + a
            out[q] = seg[a, np.arange(seg.shape[1])]
            sc[q] = np.abs(out[q])
    return out.reshape((s,) + src.shape[1:]), sc.reshape((s,) + src.shape[1:]), arg


def segment_csr_backward(dout, indptr, reduce, arg, src_shape):
    """dsrc of segment_csr: broadcast (sum), divided by the count (mean), to the arg row only (min / max)."""
    dout = np.asarray(dout, np.float64).reshape(len(indptr) - 1, -1)
    d = np.zeros((src_shape[0], dout.shape[1]))
    for q in range(len(indptr) - 1):
        lo, hi = int(indptr[q]), int(indptr[q + 1])
        if hi <= lo:
            continue
        if reduce in ("sum", "add"):
            d[lo:hi] = dout[q]
        elif reduce == "mean":
            d[lo:hi] = dout[q] / (hi - lo)
        else:
            d[arg[q], np.arange(dout.shape[1])] = dout[q]
    return d.reshape(src_shape)


def shell_cloud(n, seed, extent=160, size=(6, 40)):
    """n distinct int32 voxels [n, 3] on the faces of random hollow boxes inside [0, extent)^3, shuffled."""
    rng = np.random.default_rng(seed)
    pts = []
    v = np.zeros((0, 3), np.int64)
    while len(v) < n:
        sz = rng.integers(size[0], size[1], 3)
        lo = rng.integers(0, extent - sz, 3)
        g = np.stack(np.meshgrid(*[np.arange(s) for s in sz], indexing="ij"), -1).reshape(-1, 3)
        face = np.any((g == 0) | (g == sz - 1), axis=1)
        pts.append(g[face] + lo)
        v = np.unique(np.concatenate(pts), axis=0)
    v = v[rng.permutation(len(v))[:n]]
    return v.astype(np.int32)


def with_batch(coords, batch):
    """[N, 4] int32 indices (b, d0, d1, d2)."""
    return np.concatenate([np.asarray(batch, np.int32).reshape(-1, 1), np.asarray(coords, np.int32)], 1)


def pool_stages(coords, stages):
    """The voxel sets of successive stages: coords >> 1 and deduplicated, `stages` times."""
    out = [coords]
    for _ in range(stages):
        out.append(np.unique(out[-1] >> 1, axis=0).astype(np.int32))
    return out


# every distinct (Cin, Cout, kernel) of PTv3's 23 submanifold convolutions and the stage it runs at: the stem
# (128 -> 32, k5, stage 0) and the positional encodings of the encoder (32/64/128/256/512) and decoder stages
PTV3_SHAPES = [(128, 32, 5, 0), (32, 32, 3, 0), (64, 64, 3, 1), (128, 128, 3, 2), (256, 256, 3, 3), (512, 512, 3, 4)]
