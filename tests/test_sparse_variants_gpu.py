"""-m gpu: every kernel variant of libgcs_hip.so against the float64 reference tests/sparse_ref.py, at the smallest
shapes that select it.  test_sparse_gpu.py pins the rules at PTv3's channel counts on 16 384 rows and fewer; there the
dispatch (gcs_subm_plan) picks the 32 x 32 tile almost everywhere.  Here each test first ASSERTS the plan of its
shape, so that a moved threshold fails loudly instead of un-covering a kernel, then checks values:

  k_subm_gemm  32 x 32 / 64 x 64 / 128 x 32, forward (TRANS false) and dX (TRANS true), the 4 x 4 tiles also on
               duplicate voxels (k_fold and the row mask of dX)
  k_subm_dw    32 x 32 and 64 x 64, each with one slice and with several; k_colsum with one slice and several
  rulebook     per-axis kernel sizes and dilations (tap order, the mirror of dX), voxel keys beyond 2^32
  backward     every subset of (dx, dw, db) that autograd asks for
  segment_csr  more than one block of 64 columns, segments from 0 to 2048 rows, indptr entries outside [0, M]

Bar, as test_sparse_gpu.py: |got - ref| <= 1e-5 * scale element by element, scale = the sum of the |terms| (a float32
evaluation of the reference lies within 1.3e-7 * scale of the float64 one at these shapes, a sequential float32 sum of
2048 terms within 6.5e-8 * scale); bit-exact where the rule is a copy (one unit tap, min / max of segment_csr).

The module's name puts it after the rasteriser's GPU modules, as test_varlen_attention_gpu.py explains."""
import numpy as np
import pytest
import torch

import sparse_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("this test is marked gpu and needs a GPU; none is visible")
    from gaussiancity_amd import _native_s
    _native_s.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def S():
    from gaussiancity_amd import _native_s
    return _native_s


def _close(got, ref, scale, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > TOL * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    print("%s: worst |got - ref| / scale = %.3g" % (what, float(rel.max()) if rel.size else 0.0))
    assert not bad.any(), "%s: %d elements off, worst %g at scale %g" % (
        what, int(bad.sum()), float(err[bad].max()), float(scale[bad][np.argmax(err[bad])]))


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3


def _run(dev, idx, shape, batch, x, w, b, ksize, dil, dy, grads=(True, True, True)):
    """Forward + backward through the drop-in; y, dx, dw, db as numpy (None where `grads` freezes the input)."""
    import spconv.pytorch as spconv
    conv = spconv.SubMConv3d(x.shape[1], w.shape[0], ksize, dilation=dil, bias=b is not None).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
        if b is not None:
            conv.bias.copy_(torch.from_numpy(b))
    conv.weight.requires_grad_(grads[1])
    if b is not None:
        conv.bias.requires_grad_(grads[2])
    xt = torch.from_numpy(x).to(dev).requires_grad_(grads[0])
    out = conv(spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), batch))
    out.features.backward(torch.from_numpy(dy).to(dev))
    g = lambda p: None if p is None or p.grad is None else p.grad.cpu().numpy()  # noqa: E731
    return out.features.detach().cpu().numpy(), g(xt), g(conv.weight), g(conv.bias)


def _check_case(dev, idx, shape, batch, cin, cout, ksize, dil=1, bias=True, seed=0, what="", grads=(True, True, True)):
    """Random features, weights and dY; y and every requested gradient against the reference.  Returns (y, nbr)."""
    ksize, dil = _triple(ksize), _triple(dil)
    rng = np.random.default_rng(seed)
    n = len(idx)
    x = rng.normal(size=(n, cin)).astype(np.float32)
    w = (rng.normal(size=(cout,) + ksize + (cin,)) / np.sqrt(cin * np.prod(ksize))).astype(np.float32)
    b = rng.normal(size=cout).astype(np.float32) if bias else None
    dy = rng.normal(size=(n, cout)).astype(np.float32)
    y, dx, dw, db = _run(dev, idx, shape, batch, x, w, b, ksize, dil, dy, grads)
    nbr = R.neighbours(idx, shape, ksize, dil)
    ry, sy = R.conv_forward(x, w, b, nbr)
    (rdx, sdx), (rdw, sdw), (rdb, sdb) = R.conv_backward(x, w, nbr, dy)
    assert y.shape == (n, cout)
    _close(y, ry, sy, what + " forward")
    for got, ref, sc, name, wanted in ((dx, rdx, sdx, "dX", grads[0]), (dw, rdw, sdw, "dW", grads[1]),
                                       (db, rdb, sdb, "dB", bias and grads[2])):
        if not wanted:
            assert got is None, "%s %s: a gradient nobody asked for" % (what, name)
            continue
        assert got is not None and got.shape == ref.shape, (what, name)
        _close(got, ref, sc, "%s %s" % (what, name))
    return y, nbr


def _with_repeats(coords, count, seed):
    """The cloud plus `count` repeated rows, shuffled: several rows on one voxel."""
    rng = np.random.default_rng(seed)
    extra = coords[rng.integers(0, len(coords), count)]
    return np.concatenate([coords, extra])[rng.permutation(len(coords) + count)]


def _rows_of_one_voxel_agree(y, nbr, idx, shape, least):
    keys = R.pack(idx, shape)
    order = np.argsort(keys, kind="stable")
    same = keys[order][1:] == keys[order][:-1]
    a, b = order[1:][same], order[:-1][same]
    assert len(a) >= least
    assert np.array_equal(y[a].view(np.uint32), y[b].view(np.uint32)), "rows of one voxel differ"
    assert np.array_equal(nbr[a], nbr[b])


# ---- the two 4 x 4-per-thread tiles ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tall_cloud():
    return R.shell_cloud(32805, 2025, extent=160)


@pytest.mark.parametrize("repeats", [0, 300], ids=["distinct", "duplicates"])
def test_tall_tile_forward_and_dx(dev, S, tall_cloud, repeats):
    """128 x 32: 32 805 rows leave a partial last row tile (of 257), 20 input channels are no multiple of the 16-channel
    LDS slice, 24 and 20 output columns leave the column tile partial.  dW here is 32 x 32 in 32 slices, dB 16 slices."""
    coords = _with_repeats(tall_cloud, repeats, 1) if repeats else tall_cloud
    n, cin, cout = len(coords), 20, 24
    assert n == 32805 + repeats and n % 128 != 0
    fwd, dx, dw, dw_slices, db_slices = S.subm_plan(n, cin, cout, 27)
    assert fwd == S.TILE_128X32, "forward (%d columns) no longer takes the 128 x 32 tile" % cout
    assert dx == S.TILE_128X32, "dX (%d columns) no longer takes the 128 x 32 tile" % cin
    assert dw == S.TILE_32X32 and dw_slices > 1 and db_slices > 1
    idx = R.with_batch(coords, np.zeros(n))
    y, nbr = _check_case(dev, idx, [160] * 3, 1, cin, cout, 3, seed=3 + repeats, what="tall, %d repeats" % repeats)
    assert (nbr >= 0).sum(1).mean() > 3
    if repeats:
        _rows_of_one_voxel_agree(y, nbr, idx, [160] * 3, 250)


@pytest.fixture(scope="module")
def wide_cloud():
    return R.shell_cloud(5500, 2026, extent=80)


@pytest.mark.parametrize("repeats", [0, 550], ids=["distinct", "duplicates"])
def test_wide_tile_forward_and_dx(dev, S, wide_cloud, repeats):
    """64 x 64: 86 (95 with the repeats) x 4 tiles forward, x 3 for dX; 136 and 200 are no multiples of 64 or 16, the
    row count none of 64.  dW is the 64 x 64 kernel in several slices."""
    coords = _with_repeats(wide_cloud, repeats, 2) if repeats else wide_cloud
    n, cin, cout = len(coords), 136, 200
    assert n == 5500 + repeats and n % 64 != 0
    fwd, dx, dw, dw_slices, db_slices = S.subm_plan(n, cin, cout, 27)
    assert fwd == S.TILE_64X64, "forward (%d columns) no longer takes the 64 x 64 tile" % cout
    assert dx == S.TILE_64X64, "dX (%d columns) no longer takes the 64 x 64 tile" % cin
    assert dw == S.TILE_64X64 and dw_slices > 1 and db_slices > 1
    idx = R.with_batch(coords, np.zeros(n))
    y, nbr = _check_case(dev, idx, [80] * 3, 1, cin, cout, 3, seed=5 + repeats, what="wide, %d repeats" % repeats)
    assert (nbr >= 0).sum(1).mean() > 3
    if repeats:
        _rows_of_one_voxel_agree(y, nbr, idx, [80] * 3, 450)


@pytest.mark.parametrize("n,cin,cout,dw_tile,several", [(300, 6, 5, "TILE_32X32", False), (300, 64, 70, "TILE_64X64", False),
                                                        (700, 3, 5, "TILE_32X32", True)])
def test_small_tile_and_the_single_slice_sums(dev, S, n, cin, cout, dw_tile, several):
    """32 x 32 forward and dX under an asserted plan, and both dW kernels writing dW directly (one slice, no k_sum_slices)."""
    fwd, dx, dw, dw_slices, db_slices = S.subm_plan(n, cin, cout, 27)
    assert fwd == S.TILE_32X32 and dx == S.TILE_32X32 and dw == getattr(S, dw_tile)
    assert (dw_slices > 1) == several and db_slices == 1
    coords = R.shell_cloud(n, n + cin, extent=48)
    rng = np.random.default_rng(n)
    idx = R.with_batch(coords, rng.integers(0, 2, n))
    _check_case(dev, idx, [48] * 3, 2, cin, cout, 3, seed=cin, what="%d rows %d->%d" % (n, cin, cout))


# ---- the rulebook: per-axis geometry and the 64-bit key ------------------------------------------------------------
AXIS_KSIZE, AXIS_DIL, AXIS_SHAPE = (3, 1, 5), (1, 2, 3), [48, 40, 56]


@pytest.fixture(scope="module")
def axis_cloud():
    """About 2 000 rows in two batches inside [48, 40, 56], dense enough that the dilated taps have neighbours, some
    rows on the far faces of the grid."""
    rng = np.random.default_rng(77)
    lo = np.array(AXIS_SHAPE) - 14
    near = rng.integers(0, 14, (1400, 3))
    far = lo + rng.integers(0, 14, (1400, 3))
    idx = R.with_batch(np.concatenate([near, far]), rng.integers(0, 2, 2800))
    idx = idx[np.sort(np.unique(R.pack(idx, AXIS_SHAPE), return_index=True)[1])]
    assert 1800 <= len(idx) <= 2800 and (idx[:, 1:].max(0) == np.array(AXIS_SHAPE) - 1).all()
    return idx


def test_per_axis_kernel_and_dilation(dev, S, axis_cloud):
    assert S.subm_plan(len(axis_cloud), 5, 7, 15)[:3] == (S.TILE_32X32,) * 3
    _, nbr = _check_case(dev, axis_cloud, AXIS_SHAPE, 2, 5, 7, AXIS_KSIZE, AXIS_DIL, seed=9, what="k (3,1,5) dilation (1,2,3)")
    assert ((nbr >= 0).sum(0) > 20).all()                     # every one of the 15 taps is exercised


@pytest.mark.parametrize("tap", [0, 1, 15 // 2 - 1, 15 - 1])
def test_per_axis_one_unit_tap_is_an_exact_shift(dev, axis_cloud, tap):
    """W = identity at one tap: y is x shifted by that tap's offset and dX is dY shifted back, bit for bit.  A swapped
    axis, a wrong tap order or a wrong mirror moves other rows."""
    idx, C_, K = axis_cloud, 6, 15
    rng = np.random.default_rng(tap)
    x = rng.normal(size=(len(idx), C_)).astype(np.float32)
    dy = rng.normal(size=(len(idx), C_)).astype(np.float32)
    w = np.zeros((C_, K, C_), np.float32)
    w[np.arange(C_), tap, np.arange(C_)] = 1.0
    y, dx, _, _ = _run(dev, idx, AXIS_SHAPE, 2, x, w.reshape((C_,) + AXIS_KSIZE + (C_,)), None, AXIS_KSIZE, AXIS_DIL, dy)
    nbr = R.neighbours(idx, AXIS_SHAPE, AXIS_KSIZE, AXIS_DIL)
    # the offset of the tap, from the stated order (a * k1 + b) * k2 + c
    a, b, c = tap // 5, 0, tap % 5
    off = np.array([(a - 1) * 1, (b - 0) * 2, (c - 2) * 3])
    has = nbr[:, tap] >= 0
    assert has.sum() > 20
    assert (idx[nbr[has, tap], 1:] == idx[has, 1:] + off).all() and (idx[nbr[has, tap], 0] == idx[has, 0]).all()
    want = np.where(has[:, None], x[np.maximum(nbr[:, tap], 0)], 0.0).astype(np.float32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), tap
    want_dx = np.zeros_like(dy)
    want_dx[nbr[has, tap]] = dy[has]                           # distinct voxels: every row is the target of one row at most
    assert np.array_equal(dx.view(np.uint32), want_dx.view(np.uint32)), tap


def test_voxel_keys_beyond_32_bits(dev):
    """batch 3 x [70001, 70003, 70007] is a key space of 2^49.9.  Clusters next to both ends of every axis in every batch,
    and for some rows a second cluster whose keys differ from theirs by a multiple of 2^32: a key cut to 32 bits
    anywhere (the pack, the hash probe, the compare) merges those voxels."""
    shape, batch = [70001, 70003, 70007], 3
    rng = np.random.default_rng(64)
    rows = []
    for b in range(batch):
        for corner in range(8):
            base = np.array([(s - 4) if corner >> q & 1 else 0 for q, s in enumerate(shape)])
            pts = base + rng.integers(0, 4, (10, 3))
            rows.append(R.with_batch(pts, np.full(len(pts), b)))
    idx = np.concatenate(rows)
    s0, s1, s2 = shape
    alias = []
    for j, row in enumerate(idx[::16]):                        # keys + m * 2^32 decode to other valid voxels
        key = int(R.pack(row[None], shape)[0]) + (j + 1) * 2 ** 32
        if key + 2 >= batch * s0 * s1 * s2:
            continue
        d, c, a, b = key % s2, key // s2 % s1, key // (s2 * s1) % s0, key // (s2 * s1 * s0)
        for dd in range(-1, 2):                                # the alias and two neighbours along the last axis
            if 0 <= d + dd < s2:
                alias.append([b, a, c, d + dd])
    idx = np.concatenate([idx, np.array(alias, np.int32)]).astype(np.int32)
    idx = idx[np.sort(np.unique(R.pack(idx, shape), return_index=True)[1])]
    idx = idx[rng.permutation(len(idx))]
    keys = R.pack(idx, shape)
    low = np.sort(keys % 2 ** 32)
    assert 200 <= len(idx) <= 600 and keys.max() > 2 ** 49 and (low[1:] == low[:-1]).sum() >= 10
    for q in range(3):
        assert idx[:, q + 1].min() == 0 and idx[:, q + 1].max() == shape[q] - 1
    assert set(idx[:, 0]) == {0, 1, 2}
    _, nbr = _check_case(dev, idx, shape, batch, 4, 3, 3, seed=64, what="64-bit keys")
    assert (nbr >= 0).sum(1).mean() > 2


# ---- partial gradients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grads", [(False, True, True), (True, False, True), (True, True, False), (True, False, False)],
                         ids=["frozen-features", "frozen-weight", "frozen-bias", "features-only"])
def test_partial_gradients(dev, grads):
    """gcs_subm_backward with NULL dx, dw or db: what is produced is right, what is not asked for is not produced."""
    coords = _with_repeats(R.shell_cloud(900, 12, extent=48), 60, 12)
    idx = R.with_batch(coords, np.zeros(len(coords)))
    _check_case(dev, idx, [48] * 3, 1, 6, 5, 3, seed=12, what="grads %r" % (grads,), grads=grads)


# ---- segment_csr ---------------------------------------------------------------------------------------------------
SEG_COUNTS = [0, 2048, 1, 0, 700, 2, 63, 64, 65, 0, 1, 700, 64, 0]


def _segment_case(dev, src, indptr, indptr_ref, reduce, what):
    import torch_scatter
    rng = np.random.default_rng(len(what))
    s = torch.from_numpy(src).to(dev).requires_grad_(True)
    out = torch_scatter.segment_csr(s, torch.from_numpy(indptr).to(dev), reduce=reduce)
    dout = rng.normal(size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(dout).to(dev))
    ref, sc, arg = R.segment_csr(src, indptr_ref, reduce)
    dref = R.segment_csr_backward(dout, indptr_ref, reduce, arg, src.shape)
    got, dgot = out.detach().cpu().numpy(), s.grad.cpu().numpy()
    assert got.shape == ref.shape and dgot.shape == src.shape
    if reduce in ("min", "max"):
        assert np.array_equal(got, ref.astype(np.float32)), what
        assert np.array_equal(dgot, dref.astype(np.float32)), what + " gradient (ties go to the first row)"
    else:
        _close(got, ref, sc, what)
        dsc = R.segment_csr_backward(np.abs(dout), indptr_ref, reduce, arg, src.shape)
        _close(dgot, dref, dsc, what + " gradient")


@pytest.mark.parametrize("reduce", ["sum", "add", "mean", "min", "max"])
@pytest.mark.parametrize("trail", [(), (64,), (5, 13), (5, 26), (8, 64)], ids=["F1", "F64", "F65", "F130", "F512"])
def test_segment_csr_column_blocks_and_long_segments(dev, reduce, trail):
    """F = 1, 64 (one block of 64 columns), 65, 130 (partial last block), 512 (eight blocks); segments of 0 .. 2048 rows."""
    rng = np.random.default_rng(int(np.prod(trail, dtype=np.int64)))
    indptr = np.concatenate([[0], np.cumsum(SEG_COUNTS)]).astype(np.int64)
    m = int(indptr[-1]) + 4                      # rows after the last segment get no gradient
    src = rng.integers(-3, 4, (m,) + trail).astype(np.float32)   # small integers: many ties
    if reduce in ("sum", "add", "mean"):
        src += rng.normal(size=src.shape).astype(np.float32)
    _segment_case(dev, src, indptr, indptr, reduce, "%s F=%d" % (reduce, int(np.prod(trail, dtype=np.int64))))


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_segment_csr_clamps_indptr(dev, reduce):
    """Entries below 0 and above M are clamped to [0, M] on the device; the reference gets the clamped vector."""
    rng = np.random.default_rng(5)
    m = 150
    indptr = np.array([-9, -2, 40, 40, 111, m + 1, m + 70], np.int64)
    src = rng.integers(-3, 4, (m, 5, 13)).astype(np.float32)
    if reduce != "max":
        src += rng.normal(size=src.shape).astype(np.float32)
    _segment_case(dev, src, indptr, np.clip(indptr, 0, m), reduce, "%s, clamped indptr" % reduce)
