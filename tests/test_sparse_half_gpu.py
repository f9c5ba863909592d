"""-m gpu: the float16 path of libgcs_hip.so (GCS_F16 of the `_t` entry points, gaussiancity_amd/csrc/gcs_mfma.h, DESIGN.md
section 15): the convolution's three products on v_mfma_f32_16x16x16_f16, the binary16 fold / dB / slice sums, binary16
segment_csr, and the autocast rule of SubMConv3d.  As in test_sparse_engine_gpu.py every test first ASSERTS the plan of its
shape -- the float16 convolution launches under gcs_subm_engine_plan(GCS_ENGINE_MFMA, ...) and has no chooser of its own.

The bar.  Inputs are generated in binary16 (nonzero subnormals mapped to 0, except in the test that is about them) and
handed to tests/sparse_ref.py exactly, as float64; it returns the float64 result and A = sum |terms| (+ |bias|).  One UNIT
is 2^-11 * A + 2^-24: the rounding of the final store plus half the subnormal spacing twice over.  y, dX, dW, dB and
segment_csr sum / mean: 2 units on every element (one for the store, one of room for the fp32 accumulation order; the
fp32-accumulate, round-once formulation alone stays below 1 unit on these shapes, test_sparse_half_host.py).  dX and dW on a
cloud with duplicates: 3 units (the binary16 fold).  mean's backward: 1 unit of |dout| / count.  What the contract calls
exact is compared bit for bit.  Every check prints its worst ratio before it asserts.

The module's name puts it after the rasteriser's GPU modules, as test_varlen_attention_gpu.py explains."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import sparse_ref as R
import test_sparse_variants_gpu as V

pytestmark = pytest.mark.gpu
AXIS_KSIZE, AXIS_DIL, AXIS_SHAPE = V.AXIS_KSIZE, V.AXIS_DIL, V.AXIS_SHAPE


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


def _h(a):
    """binary16 of `a`, nonzero subnormals mapped to 0."""
    h = np.asarray(a).astype(np.float16)
    h[np.abs(h.astype(np.float32)) < 2.0 ** -14] = 0
    return h


def _f64(a):
    return None if a is None else np.asarray(a).astype(np.float64)


def _bits(a):
    assert a.dtype == np.float16
    return np.ascontiguousarray(a).view(np.uint16)


def _units(got, ref, scale, what, bar):
    assert got.dtype == np.float16, (what, got.dtype)
    assert np.isfinite(got.astype(np.float32)).all(), what + ": not finite"
    ratio = np.abs(got.astype(np.float64) - ref) / (2.0 ** -11 * scale + 2.0 ** -24)
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%s: worst |got - float64| / unit = %.3f (bar %g)" % (what, worst, bar))
    assert worst <= bar, "%s: %d elements beyond %g units, worst %.3f" % (what, int((ratio > bar).sum()), bar, worst)
    return worst


def _run(dev, idx, shape, batch, x, w, b, ksize, dil, dy, grads=(True, True, True)):
    """Forward + backward through a .half() layer; y, dx, dw, db as float16 numpy (None where `grads` freezes the input)."""
    import spconv.pytorch as spconv
    assert x.dtype == w.dtype == dy.dtype == np.float16
    conv = spconv.SubMConv3d(x.shape[1], w.shape[0], ksize, dilation=dil, bias=b is not None).to(dev).half()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
        if b is not None:
            conv.bias.copy_(torch.from_numpy(b))
    conv.weight.requires_grad_(grads[1])
    if b is not None:
        conv.bias.requires_grad_(grads[2])
    xt = torch.from_numpy(x).to(dev).requires_grad_(grads[0])
    out = conv(spconv.SparseConvTensor(xt, torch.from_numpy(idx).to(dev), list(shape), batch))
    assert out.features.dtype == torch.float16
    out.features.backward(torch.from_numpy(dy).to(dev))
    g = lambda p: None if p is None or p.grad is None else p.grad.cpu().numpy()  # noqa: E731
    got = out.features.detach().cpu().numpy(), g(xt), g(conv.weight), g(conv.bias)
    for t in got:
        assert t is None or t.dtype == np.float16
    return got


def _check_case(dev, idx, shape, batch, cin, cout, ksize, dil=1, bias=True, seed=0, what="", grads=(True, True, True),
                dups=False):
    """Random binary16 features, weights, bias and dY; y and every requested gradient against float64.  Returns (y, nbr)."""
    ksize, dil = V._triple(ksize), V._triple(dil)
    rng = np.random.default_rng(seed)
    n = len(idx)
    x = _h(rng.normal(size=(n, cin)))
    w = _h(rng.normal(size=(cout,) + ksize + (cin,)) / np.sqrt(cin * np.prod(ksize)))
    b = _h(rng.normal(size=cout)) if bias else None
    dy = _h(rng.normal(size=(n, cout)))
    y, dx, dw, db = _run(dev, idx, shape, batch, x, w, b, ksize, dil, dy, grads)
    nbr = R.neighbours(idx, shape, ksize, dil)
    ry, sy = R.conv_forward(_f64(x), _f64(w), _f64(b), nbr)
    (rdx, sdx), (rdw, sdw), (rdb, sdb) = R.conv_backward(_f64(x), _f64(w), nbr, _f64(dy))
    assert y.shape == (n, cout)
    _units(y, ry, sy, what + " y", 2)
    wide = 3 if dups else 2
    for got, ref, sc, name, wanted, bar in ((dx, rdx, sdx, "dX", grads[0], wide), (dw, rdw, sdw, "dW", grads[1], wide),
                                            (db, rdb, sdb, "dB", bias and grads[2], 2)):
        if not wanted:
            assert got is None, "%s %s: a gradient nobody asked for" % (what, name)
            continue
        assert got is not None and got.shape == ref.shape, (what, name)
        _units(got, ref, sc, "%s %s" % (what, name), bar)
    if dups and grads[0]:                                       # dX of a row that is not its voxel's representative is 0
        others = nbr[:, nbr.shape[1] // 2] != np.arange(n)
        assert others.sum() >= 50 and not np.any(_bits(dx[others]) & 0x7FFF), what + ": dX of a non-representative row"
    return y, nbr


def _plan(S, n, cin, cout, K):
    return S.subm_engine_plan(S.ENGINE_MFMA, n, cin, cout, K)


def _axis_rows(count, seed):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(0, s, 3 * count) for s in AXIS_SHAPE], 1)
    idx = R.with_batch(pts, rng.integers(0, 2, len(pts)))
    idx = idx[np.sort(np.unique(R.pack(idx, AXIS_SHAPE), return_index=True)[1])][:count]
    assert len(idx) == count
    return idx


@pytest.fixture(scope="module")
def axis_cloud():
    """The cloud of test_sparse_variants_gpu.py's axis tests: 2 469 rows, dense enough for the dilated taps."""
    rng = np.random.default_rng(77)
    lo = np.array(AXIS_SHAPE) - 14
    near = rng.integers(0, 14, (1400, 3))
    far = lo + rng.integers(0, 14, (1400, 3))
    idx = R.with_batch(np.concatenate([near, far]), rng.integers(0, 2, 2800))
    idx = idx[np.sort(np.unique(R.pack(idx, AXIS_SHAPE), return_index=True)[1])]
    assert len(idx) == 2469
    return idx


@pytest.fixture(scope="module")
def shell():
    return R.pool_stages(R.shell_cloud(16384, 2024), 4)


# ---- 1. operand maps, exactly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap", [0, 6, 14])
@pytest.mark.parametrize("sliced", [False, True], ids=["one-slice", "sliced"])
def test_selection_weight_is_an_exact_copy(dev, S, axis_cloud, sliced, tap):
    """cin = 37: every second row of x starts at an odd 2-byte offset, and no 8-byte load is possible."""
    cin, cout, K = 37, 21, 15
    idx = axis_cloud if sliced else _axis_rows(9000, 5)
    n = len(idx)
    fs, xs = _plan(S, n, cin, cout, K)[5:]
    assert (fs > 1 and xs > 1) if sliced else (fs, xs) == (1, 1), (n, fs, xs)
    rng = np.random.default_rng(tap + 100 * sliced)
    x, dy = _h(rng.normal(size=(n, cin))), _h(rng.normal(size=(n, cout)))
    sel = (3 * np.arange(cout) + 1) % cin                      # output o reads input channel sel[o]; injective
    assert len(set(sel)) == cout and not np.array_equal(sel, np.arange(cout))
    w = np.zeros((cout, K, cin), np.float16)
    w[np.arange(cout), tap, sel] = 1.0
    y, dx, _, _ = _run(dev, idx, AXIS_SHAPE, 2, x, w.reshape((cout,) + AXIS_KSIZE + (cin,)), None, AXIS_KSIZE, AXIS_DIL, dy)
    nbr = R.neighbours(idx, AXIS_SHAPE, AXIS_KSIZE, AXIS_DIL)
    has = nbr[:, tap] >= 0
    assert has.sum() > 20
    want = np.where(has[:, None], x[np.maximum(nbr[:, tap], 0)][:, sel], 0.0).astype(np.float16)
    assert np.array_equal(_bits(y), _bits(want)), "forward, tap %d" % tap
    want_dx = np.zeros((n, cin), np.float16)
    rows = np.nonzero(has)[0]
    want_dx[nbr[rows, tap][:, None], sel[None, :]] = dy[rows]   # distinct voxels: one source row per target at most
    assert np.array_equal(_bits(dx), _bits(want_dx)), "dX, tap %d" % tap


# ---- 2. dW: exact integer sums ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,dw_tile,several", [(300, 6, 5, "TILE_32X32", False), (700, 3, 5, "TILE_32X32", True),
                                                        (300, 64, 70, "TILE_64X64", False)])
def test_dw_integer_sums_are_exact(dev, S, n, cin, cout, dw_tile, several):
    plan = _plan(S, n, cin, cout, 27)
    assert plan[2] == getattr(S, dw_tile) and (plan[3] > 1) == several, plan
    coords = R.shell_cloud(n, n + cin, extent=48)
    rng = np.random.default_rng(n + cout)
    idx = R.with_batch(coords, rng.integers(0, 2, n))
    x = rng.integers(-2, 3, (n, cin)).astype(np.float16)
    ostar = cout - 2
    dy = np.zeros((n, cout), np.float16)
    dy[::64, ostar] = rng.choice([-1.0, 1.0], len(dy[::64]))
    w = _h(rng.normal(size=(cout, 3, 3, 3, cin)) / 9)
    nbr = R.neighbours(idx, [48] * 3, (3, 3, 3), (1, 1, 1))
    (_, _), (want, _), _ = R.conv_backward(_f64(x), _f64(w), nbr, _f64(dy))
    assert np.abs(want).max() <= 2048 and np.abs(want).max() >= 2 and np.array_equal(want, np.round(want))
    _, _, dw, _ = _run(dev, idx, [48] * 3, 2, x, w, None, (3, 3, 3), (1, 1, 1), dy)
    assert np.array_equal(_bits(dw), _bits(want.astype(np.float16))), "dW differs from the integer sums"
    others = np.delete(dw, ostar, axis=0)
    assert not np.any(_bits(others) & 0x7FFF), "a dW row other than o* is not zero"


# ---- 3. the float64 bar on every tile ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,dw_tile", [(300, 6, 5, "TILE_32X32"), (300, 64, 70, "TILE_64X64")])
def test_small_tiles(dev, S, n, cin, cout, dw_tile):
    plan = _plan(S, n, cin, cout, 27)
    assert plan[0] == plan[1] == S.TILE_32X32 and plan[2] == getattr(S, dw_tile) and plan[5] > 1 and plan[6] > 1, plan
    coords = R.shell_cloud(n, n + cin, extent=48)
    idx = R.with_batch(coords, np.random.default_rng(n).integers(0, 2, n))
    _check_case(dev, idx, [48] * 3, 2, cin, cout, 3, seed=cin, what="%d rows %d->%d" % (n, cin, cout))


@pytest.fixture(scope="module")
def wide_cloud():
    return R.shell_cloud(5500, 2026, extent=80)


@pytest.mark.parametrize("repeats", [0, 550], ids=["distinct", "duplicates"])
def test_wide_tile(dev, S, wide_cloud, repeats):
    coords = V._with_repeats(wide_cloud, repeats, 2) if repeats else wide_cloud
    n, cin, cout = len(coords), 136, 200
    plan = _plan(S, n, cin, cout, 27)
    assert plan[0] == plan[1] == plan[2] == S.TILE_64X64 and plan[3] > 1 and plan[4] > 1 and plan[5:] == (1, 1), plan
    idx = R.with_batch(coords, np.zeros(n))
    y, nbr = _check_case(dev, idx, [80] * 3, 1, cin, cout, 3, seed=5 + repeats, what="wide, %d repeats" % repeats,
                         dups=bool(repeats))
    if repeats:
        _rows_of_one_voxel_agree(y, nbr, idx, [80] * 3, 450)


@pytest.fixture(scope="module")
def tall_cloud():
    return R.shell_cloud(32805, 2025, extent=160)


@pytest.mark.parametrize("repeats", [0, 300], ids=["distinct", "duplicates"])
def test_tall_tile(dev, S, tall_cloud, repeats):
    coords = V._with_repeats(tall_cloud, repeats, 1) if repeats else tall_cloud
    n, cin, cout = len(coords), 20, 24
    plan = _plan(S, n, cin, cout, 27)
    assert plan[0] == plan[1] == S.TILE_128X32 and plan[2] == S.TILE_32X32 and plan[3] > 1 and plan[4] > 1, plan
    idx = R.with_batch(coords, np.zeros(n))
    y, nbr = _check_case(dev, idx, [160] * 3, 1, cin, cout, 3, seed=3 + repeats, what="tall, %d repeats" % repeats,
                         dups=bool(repeats))
    if repeats:
        _rows_of_one_voxel_agree(y, nbr, idx, [160] * 3, 250)


def _rows_of_one_voxel_agree(y, nbr, idx, shape, least):
    keys = R.pack(idx, shape)
    order = np.argsort(keys, kind="stable")
    same = keys[order][1:] == keys[order][:-1]
    a, b = order[1:][same], order[:-1][same]
    assert len(a) >= least
    assert np.array_equal(_bits(y[a]), _bits(y[b])), "rows of one voxel differ"


def test_axis_cloud_fifteen_taps(dev, S, axis_cloud):
    plan = _plan(S, len(axis_cloud), 5, 7, 15)
    assert plan[:3] == (S.TILE_32X32,) * 3 and plan[5] > 1 and plan[6] > 1, plan
    _, nbr = _check_case(dev, axis_cloud, AXIS_SHAPE, 2, 5, 7, AXIS_KSIZE, AXIS_DIL, seed=9, what="axis cloud 5->7, K = 15")
    assert ((nbr >= 0).sum(0) > 20).all()


# ---- 4. determinism and workspace independence, through the C ABI -------------------------------------------------------
@pytest.mark.parametrize("sliced", [True, False], ids=["sliced", "one-slice"])
def test_workspace_contents_stream_and_repetition_do_not_change_a_bit(dev, S, axis_cloud, sliced):
    from gaussiancity_amd import sparse as SP
    cin, cout, K = (5, 7, 15) if sliced else (37, 21, 15)
    idx_np = axis_cloud if sliced else _axis_rows(9000, 5)
    n = len(idx_np)
    plan = _plan(S, n, cin, cout, K)
    assert (plan[5] > 1 and plan[6] > 1) if sliced else plan[5:] == (1, 1), plan
    fwd_bytes, bwd_bytes = S.subm_workspace_bytes_t(S.DTYPE_F16, n, cin, cout, K, 0)
    assert (fwd_bytes > 0) == sliced and bwd_bytes > 0
    rng = np.random.default_rng(4 + sliced)
    xn, dyn = _h(rng.normal(size=(n, cin))), _h(rng.normal(size=(n, cout)))
    wn, bn = _h(rng.normal(size=(cout, K, cin)) / np.sqrt(K * cin)), _h(rng.normal(size=cout))
    x, dy, w, b = (torch.from_numpy(a).to(dev) for a in (xn, dyn, wn, bn))
    idx = torch.from_numpy(idx_np).to(dev)
    rb = SP.Rulebook(idx, AXIS_SHAPE, 2, AXIS_KSIZE, AXIS_DIL)
    assert rb.dups == 0
    L = S.lib()
    second = torch.cuda.Stream(device=dev)
    results = []
    for fill, stream in ((0xFF, None), (0x00, None), (0xFF, second), (0xFF, None)):
        ws_f = torch.full((max(fwd_bytes, 1),), fill, dtype=torch.uint8, device=dev)
        ws_b = torch.full((bwd_bytes,), fill, dtype=torch.uint8, device=dev)
        y = torch.full((n, cout), 7.0, device=dev, dtype=torch.float16)
        dx = torch.full((n, cin), 7.0, device=dev, dtype=torch.float16)
        dw = torch.full((cout, K, cin), 7.0, device=dev, dtype=torch.float16)
        db = torch.full((cout,), 7.0, device=dev, dtype=torch.float16)
        torch.cuda.synchronize()
        st = C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        S.check(L.gcs_subm_forward_t(S.DTYPE_F16, rb.buf.data_ptr(), n, K, x.data_ptr(), cin, w.data_ptr(), b.data_ptr(),
                                     cout, y.data_ptr(), ws_f.data_ptr() if fwd_bytes else None, fwd_bytes, st), "forward")
        S.check(L.gcs_subm_backward_t(S.DTYPE_F16, rb.buf.data_ptr(), n, K, 0, x.data_ptr(), cin, w.data_ptr(), cout,
                                      dy.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws_b.data_ptr(),
                                      bwd_bytes, st), "backward")
        torch.cuda.synchronize()
        results.append([t.cpu().numpy() for t in (y, dx, dw, db)])
    for other in results[1:]:
        for name, a, c in zip(("y", "dX", "dW", "dB"), results[0], other):
            assert np.array_equal(_bits(a), _bits(c)), name + " depends on the workspace, the stream or the run"
    nbr = R.neighbours(idx_np, AXIS_SHAPE, AXIS_KSIZE, AXIS_DIL)
    w5 = _f64(wn).reshape((cout,) + AXIS_KSIZE + (cin,))
    ry, sy = R.conv_forward(_f64(xn), w5, _f64(bn), nbr)
    (rdx, sdx), (rdw, sdw), (rdb, sdb) = R.conv_backward(_f64(xn), w5, nbr, _f64(dyn))
    y, dx, dw, db = results[0]
    _units(y, ry, sy, "C ABI y", 2)
    _units(dx, rdx, sdx, "C ABI dX", 2)
    _units(dw.reshape(rdw.shape), rdw, sdw, "C ABI dW", 2)
    _units(db, rdb, sdb, "C ABI dB", 2)


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------
def test_an_empty_cloud(dev):
    import spconv.pytorch as spconv
    conv = spconv.SubMConv3d(4, 3, 3).to(dev).half()
    x = torch.zeros((0, 4), dtype=torch.float16, device=dev, requires_grad=True)
    out = conv(spconv.SparseConvTensor(x, torch.zeros((0, 4), dtype=torch.int32, device=dev), [5, 6, 7], 2))
    assert out.features.dtype == torch.float16 and tuple(out.features.shape) == (0, 3)
    out.features.backward(torch.zeros((0, 3), dtype=torch.float16, device=dev))
    assert tuple(x.grad.shape) == (0, 4)
    assert conv.weight.grad.dtype == torch.float16 and not conv.weight.grad.any() and not conv.bias.grad.any()


def _repeated_cloud():
    coords = V._with_repeats(R.shell_cloud(900, 12, extent=48), 60, 12)
    return R.with_batch(coords, np.zeros(len(coords)))


@pytest.mark.parametrize("grads", [g for g in itertools.product((True, False), repeat=3) if any(g)],
                         ids=lambda g: "".join(n for n, on in zip(("dx", "dw", "db"), g) if on))
def test_every_subset_of_gradients(dev, grads):
    _check_case(dev, _repeated_cloud(), [48] * 3, 1, 24, 40, 3, seed=12, what="grads %r" % (grads,), grads=grads, dups=True)


def test_a_float_layer_and_a_half_layer_share_one_rulebook(dev):
    import spconv.pytorch as spconv
    from gaussiancity_amd import sparse as SP
    coords = R.shell_cloud(2000, 3, extent=50)
    idx_np = R.with_batch(coords, np.zeros(len(coords)))
    x = _h(np.random.default_rng(8).normal(size=(len(coords), 8)))
    idx = torch.from_numpy(idx_np).to(dev)
    t32 = spconv.SparseConvTensor(torch.from_numpy(x.astype(np.float32)).to(dev), idx, [50, 50, 50], 1)
    a = spconv.SubMConv3d(8, 8, 3, indice_key="s0").to(dev)
    b = spconv.SubMConv3d(8, 8, 3, indice_key="s0").to(dev).half()
    SP.reset_stats()
    ya = a(t32)
    before = SP.stats()
    assert before["rulebook_builds"] == 1 and before["conv_forward_calls_half"] == 0
    t16 = ya.replace_feature(torch.from_numpy(x).to(dev).requires_grad_(True))
    yb = b(t16)
    yb.features.sum().backward()
    st = SP.stats()
    assert st["rulebook_builds"] == 1 and yb.indice_dict is t32.indice_dict
    assert (st["conv_forward_calls_half"], st["conv_dw_calls_half"]) == (1, 1)
    for key in ("conv_forward_calls_valu", "conv_forward_calls_mfma", "conv_dw_calls_valu", "conv_dw_calls_mfma"):
        assert st[key] == before[key], key
    nbr = R.neighbours(idx_np, [50] * 3, (3, 3, 3), (1, 1, 1))
    ry, sy = R.conv_forward(_f64(x), _f64(b.weight.detach().cpu().numpy()), _f64(b.bias.detach().cpu().numpy()), nbr)
    _units(yb.features.detach().cpu().numpy(), ry, sy, "shared rulebook, half layer", 2)
    ry, sy = R.conv_forward(_f64(x), _f64(a.weight.detach().cpu().numpy()), _f64(a.bias.detach().cpu().numpy()), nbr)
    V._close(ya.features.detach().cpu().numpy(), ry, sy, "shared rulebook, float layer")


def test_the_engine_setting_does_not_touch_a_half_layer(dev, shell):
    import spconv.pytorch as spconv
    from gaussiancity_amd import sparse as SP
    coords = shell[2]
    n = len(coords)
    conv = spconv.SubMConv3d(24, 40, 3).to(dev).half()
    x = torch.from_numpy(_h(np.random.default_rng(1).normal(size=(n, 24)))).to(dev)
    idx = torch.from_numpy(R.with_batch(coords, np.zeros(n))).to(dev)
    shape = (coords.max(0) + 3).tolist()
    outs = []
    start = SP.get_engine()
    try:
        for name in ("valu", "mfma", "valu"):
            SP.set_engine(name)
            outs.append(conv(spconv.SparseConvTensor(x, idx, shape, 1)).features.detach().cpu().numpy())
    finally:
        SP.set_engine(start)
    assert np.abs(outs[0].astype(np.float32)).max() > 0
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))


# ---- 6. autocast -----------------------------------------------------------------------------------------------------------
class _CPE(torch.nn.Module):
    """The shape of a PTv3 block's conditional positional encoding: SubMConv3d -> Linear -> LayerNorm."""

    def __init__(self, c):
        super().__init__()
        import spconv.pytorch as spconv
        self.conv = spconv.SubMConv3d(c, c, 3, indice_key="cpe")
        self.lin = torch.nn.Linear(c, c)
        self.norm = torch.nn.LayerNorm(c)

    def forward(self, t):
        t = self.conv(t)
        return t, self.norm(self.lin(t.features))


@pytest.mark.parametrize("ac_dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_autocast_as_spconv_does_it(dev, shell, ac_dtype):
    import spconv.pytorch as spconv
    coords = shell[1]
    n, c = len(coords), 32
    assert n == 4292
    torch.manual_seed(6)
    block = _CPE(c).to(dev)
    x32 = torch.randn(n, c, device=dev)
    idx = torch.from_numpy(R.with_batch(coords, np.zeros(n))).to(dev)
    shape = (coords.max(0) + 3).tolist()
    x = x32.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=ac_dtype):
        t, out = block(spconv.SparseConvTensor(x, idx, shape, 1))
        loss = out.float().square().mean()
    assert t.features.dtype == torch.float16, "the conv output under autocast is float16, whatever the autocast dtype"
    loss.backward()
    for name, p in block.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), name
    assert x.grad.dtype == torch.float32 and torch.isfinite(x.grad).all()
    assert block.conv.weight.grad.abs().max() > 0 and x.grad.abs().max() > 0
    assert not torch.is_autocast_enabled()
    explicit = spconv.SubMConv3d(c, c, 3).to(dev).half()
    with torch.no_grad():
        explicit.weight.copy_(block.conv.weight.half())
        explicit.bias.copy_(block.conv.bias.half())
        want = explicit(spconv.SparseConvTensor(x32.half(), idx, shape, 1)).features
    assert torch.equal(t.features.detach().view(torch.int16), want.view(torch.int16)), "autocast differs from the explicit half call"
    # features of another floating dtype (what a Linear emits under bfloat16 autocast) are cast too, as custom_fwd does
    xb = x32.bfloat16()
    with torch.autocast("cuda", dtype=ac_dtype), torch.no_grad():
        got = block.conv(spconv.SparseConvTensor(xb, idx, shape, 1)).features
        want = explicit(spconv.SparseConvTensor(xb.half(), idx, shape, 1)).features
    assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    with pytest.raises(TypeError):                              # outside autocast bfloat16 stays refused
        block.conv(spconv.SparseConvTensor(xb, idx, shape, 1))


# ---- 7. segment_csr ---------------------------------------------------------------------------------------------------------
SEG_COUNTS = V.SEG_COUNTS
TRAILS = [(), (64,), (5, 13), (5, 26), (8, 64)]


@pytest.fixture(scope="module")
def seg_indptr():
    """SEG_COUNTS with an entry below 0 in front and one beyond M at the end: the device clamps, the reference gets the
    clamped vector.  M is 4 rows beyond the last counted segment: the last segment owns them after the clamp."""
    inner = np.concatenate([[0], np.cumsum(SEG_COUNTS)]).astype(np.int64)
    m = int(inner[-1]) + 4
    indptr = np.concatenate([[-9], inner, [m + 70]]).astype(np.int64)
    return indptr, np.clip(indptr, 0, m), m


@pytest.mark.parametrize("reduce", ["sum", "mean", "min", "max"])
@pytest.mark.parametrize("trail", TRAILS, ids=["F1", "F64", "F65", "F130", "F512"])
def test_segment_csr_half(dev, seg_indptr, reduce, trail):
    import torch_scatter
    indptr, clamped, m = seg_indptr
    f = int(np.prod(trail, dtype=np.int64))
    rng = np.random.default_rng(f + len(reduce))
    if reduce in ("min", "max"):
        values = np.array([-3, -1.5, -0.25, 0, 0.25, 1, 2.5, 3], np.float16)      # at most 8 distinct values: ties
        src = values[rng.integers(0, 8, (m,) + trail)]
    else:
        src = _h(rng.normal(size=(m,) + trail))
    ref, sc, arg = R.segment_csr(_f64(src), clamped, reduce)
    nseg = len(indptr) - 1
    if reduce in ("min", "max"):
        flat = src.reshape(m, -1)
        tied = sum(1 for q in range(nseg) if clamped[q + 1] > clamped[q]
                   and ((flat[clamped[q]:clamped[q + 1]] == ref.reshape(nseg, -1)[q].astype(np.float16)).sum(0) > 1).any())
        assert 4 * tied >= nseg, "only %d of %d segments have a tie" % (tied, nseg)
    s = torch.from_numpy(src).to(dev).requires_grad_(True)
    out = torch_scatter.segment_csr(s, torch.from_numpy(indptr).to(dev), reduce=reduce)
    assert out.dtype == torch.float16 and tuple(out.shape) == (nseg,) + trail
    dout = _h(rng.normal(size=tuple(out.shape)))
    out.backward(torch.from_numpy(dout).to(dev))
    got, dgot = out.detach().cpu().numpy(), s.grad.cpu().numpy()
    assert dgot.dtype == np.float16 and dgot.shape == src.shape
    what = "segment_csr %s F=%d" % (reduce, f)
    empty = clamped[1:] == clamped[:-1]
    assert empty.sum() >= 4 and not np.any(_bits(got[empty]) & 0x7FFF), what + ": an empty segment is not 0"
    dref = R.segment_csr_backward(_f64(dout), clamped, reduce, arg, src.shape)
    if reduce in ("min", "max"):
        assert np.array_equal(_bits(got), _bits(ref.astype(np.float16))), what
        assert np.array_equal(_bits(dgot), _bits(dref.astype(np.float16))), what + " gradient (ties go to the first row)"
    elif reduce == "sum":
        _units(got, ref, sc, what, 2)
        assert np.array_equal(_bits(dgot), _bits(dref.astype(np.float16))), what + " gradient is a copy"
    else:
        _units(got, ref, sc, what, 2)
        _units(dgot, dref, np.abs(dref), what + " gradient", 1)


@pytest.mark.parametrize("reduce", ["min", "max"])
def test_segment_csr_arg_through_the_c_abi(dev, S, seg_indptr, reduce):
    """`arg` itself: the FIRST row attaining the value, -1 for an empty segment (the autograd layer keeps it to itself)."""
    indptr, clamped, m = seg_indptr
    f, nseg = 65, len(indptr) - 1
    rng = np.random.default_rng(65)
    values = np.array([-3, -1.5, -0.25, 0, 0.25, 1, 2.5, 3], np.float16)
    src = values[rng.integers(0, 8, (m, f))]
    ref, _, arg = R.segment_csr(_f64(src), clamped, reduce)
    assert (arg == -1).any() and (arg >= 0).any()
    s, ip = torch.from_numpy(src).to(dev), torch.from_numpy(indptr).to(dev)
    out = torch.full((nseg, f), 7.0, dtype=torch.float16, device=dev)
    got_arg = torch.full((nseg, f), -7, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    S.check(S.lib().gcs_segment_csr_forward_t(S.DTYPE_F16, s.data_ptr(), m, f, ip.data_ptr(), nseg, S.REDUCE[reduce],
                                              out.data_ptr(), got_arg.data_ptr(), st), "gcs_segment_csr_forward_t")
    torch.cuda.synchronize()
    assert np.array_equal(got_arg.cpu().numpy(), arg), "arg is not the first attaining row"
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref.astype(np.float16)))


# ---- 8. subnormal operands ------------------------------------------------------------------------------------------------
def test_subnormal_operands_are_exact_or_read_as_zero(dev):
    """x = integers * 2^-20 (binary16 subnormals), w = 2^10 on the centre tap: every y is integer * 2^-10 when the matrix
    cores read subnormal operands, 0 when they flush them.  Either is accepted, the same for every element; prints which.
    dX likewise, with dY subnormal."""
    n, c = 300, 16
    coords = R.shell_cloud(n, 41, extent=48)
    idx = R.with_batch(coords, np.zeros(n))
    rng = np.random.default_rng(20)
    ints = rng.integers(1, 64, (n, c)) * rng.choice([-1, 1], (n, c))
    x = (ints * 2.0 ** -20).astype(np.float16)
    assert np.array_equal(x.astype(np.float64), ints * 2.0 ** -20) and (np.abs(x.astype(np.float32)) < 2.0 ** -14).all()
    w = np.zeros((c, 27, c), np.float16)
    w[np.arange(c), 13, np.arange(c)] = 1024.0
    y, dx, _, _ = _run(dev, idx, [48] * 3, 1, x, w.reshape(c, 3, 3, 3, c), None, (3, 3, 3), (1, 1, 1), x)
    exact = (ints * 2.0 ** -10).astype(np.float16)
    for name, got in (("y", y), ("dX", dx)):
        if np.array_equal(_bits(got), _bits(exact)):
            print("subnormal operands, %s: v_mfma_f32_16x16x16_f16 reads them exactly" % name)
        elif not np.any(_bits(got) & 0x7FFF):
            print("subnormal operands, %s: v_mfma_f32_16x16x16_f16 reads them as 0" % name)
        else:
            pytest.fail("%s: neither exact nor flushed in every element (%d exact, %d zero of %d)" % (
                name, int((got == exact).sum()), int((got == 0).sum()), got.size))


# ---- 9. reading float32 operands and rounding the result is not the contract -------------------------------------------
def test_operands_are_rounded_to_binary16_before_the_products(dev):
    """float32 x and w through autocast.  Rounding normal operands to nearest moves a product by 2^-10 of itself at most,
    about 2 units of the sum, so that alone cannot separate "operands rounded first" from "float32 operands, result
    rounded" by the 4 units asked for here.  Channel 0 therefore holds x in [2^-26, 2^-25), which binary16 rounds to ZERO (not
    to a subnormal), against w in [2^15, 2^16): a term of 2^-11 or more per present tap that only unrounded operands see."""
    import spconv.pytorch as spconv
    n, cin, cout = 300, 6, 5
    coords = R.shell_cloud(n, n + cin, extent=48)
    idx = R.with_batch(coords, np.random.default_rng(n).integers(0, 2, n))
    rng = np.random.default_rng(99)
    x32 = rng.normal(size=(n, cin)).astype(np.float32)
    w32 = (rng.normal(size=(cout, 3, 3, 3, cin)) / np.sqrt(27 * cin)).astype(np.float32)
    for a in (x32, w32):
        a[np.abs(a) < 2.0 ** -13] = 0                           # no binary16 subnormals after the cast
    x32[:, 0] = (2.0 ** -26 * rng.uniform(1.0, 1.99, n)).astype(np.float32)
    w32[..., 0] = (2.0 ** 15 * rng.uniform(1.0, 1.9, w32.shape[:-1])).astype(np.float32)
    xh, wh = x32.astype(np.float16), w32.astype(np.float16)
    assert (xh.astype(np.float32) != x32).mean() > 0.9 and (wh.astype(np.float32) != w32).mean() > 0.9
    assert not xh[:, 0].any() and np.isfinite(wh.astype(np.float32)).all()
    for a in (xh, wh):
        assert not ((a != 0) & (np.abs(a.astype(np.float32)) < 2.0 ** -14)).any()
    nbr = R.neighbours(idx, [48] * 3, (3, 3, 3), (1, 1, 1))
    r_round, s_round = R.conv_forward(_f64(xh), _f64(wh), None, nbr)
    r_plain, _ = R.conv_forward(_f64(x32), _f64(w32), None, nbr)
    unit = 2.0 ** -11 * s_round + 2.0 ** -24
    assert (np.abs(r_round - r_plain) / unit).max() > 4, "the two references are too close to tell the paths apart"
    conv = spconv.SubMConv3d(cin, cout, 3, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w32))
    with torch.autocast("cuda", dtype=torch.float16):
        y = conv(spconv.SparseConvTensor(torch.from_numpy(x32).to(dev), torch.from_numpy(idx).to(dev), [48] * 3, 2)).features
    y = y.detach().cpu().numpy()
    _units(y, r_round, s_round, "autocast y against the rounded operands", 2)
    off = (np.abs(y.astype(np.float64) - r_plain) / unit).max()
    print("autocast y against the unrounded operands: worst %.3f units" % off)
    assert off > 2, "y matches the float32 operands: they were not rounded to binary16 first"
