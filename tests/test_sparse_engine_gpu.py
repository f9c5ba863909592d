"""-m gpu: the matrix-core engine of the submanifold convolution (GCS_ENGINE_MFMA: k_subm_gemm_mfma and the tap slices,
gaussiancity_amd/csrc/gcs_mfma.h) against the VALU engine and the float64 reference
tests/sparse_ref.py.  As in test_sparse_variants_gpu.py every test first ASSERTS the plan of its shape
(gcs_subm_engine_plan), so that a moved threshold fails loudly instead of un-covering a path, and every test restores the
engine it found.

  operand maps   a selection weight that is not symmetric (W[o][tap][c] = 1 iff c == (3 o + 1) mod cin): y and dX are
                 copies, bit for bit, with one slice and with several; a transposed fragment, a swapped row / column of
                 the C/D store or a wrong mirror moves values
  equality       where the plan has ONE tap slice the engine keeps the VALU engine's summation order, and the f32 MFMA is
                 a k-ordered fmaf chain: y and dX are equal as float values, on all three tiles, with duplicates too
  sliced shapes  y, dX, dW, dB against float64 under the project's bar, |got - ref| <= 1e-5 * sum |terms|
  determinism    through the C ABI: the workspace's previous contents and the stream do not change a bit
  plumbing       n == 0, every subset of gradients, the engine of a layer's backward, rulebooks shared across engines

The 300-row 6 -> 5 shape of test_sparse_variants_gpu.py has a tile grid of 10 workgroups, so the plan cuts it into tap
slices: its partial chains are summed afterwards and equality with the VALU engine is not defined for it.  It is held to
the float64 bar here, and the 32 x 32 tile's equality is checked at 8 200 rows, where the plan has one slice.

The module's name puts it after the rasteriser's GPU modules, as test_varlen_attention_gpu.py explains."""
import contextlib
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


@contextlib.contextmanager
def engine(name):
    from gaussiancity_amd import sparse as SP
    prev = SP.set_engine(name)
    try:
        yield
    finally:
        SP.set_engine(prev)


def _slices(S, n, cin, cout, K):
    """(forward slices, dX slices) of the matrix-core engine; its tiles must be the VALU plan's."""
    plan = S.subm_engine_plan(S.ENGINE_MFMA, n, cin, cout, K)
    assert plan[:5] == S.subm_plan(n, cin, cout, K)
    return plan[5], plan[6]


def _axis_rows(count, seed):
    """`count` distinct voxels in two batches inside AXIS_SHAPE, uniformly spread, some on the far faces."""
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
    assert 1800 <= len(idx) <= 2800
    return idx


@pytest.fixture(scope="module")
def shell():
    return R.pool_stages(R.shell_cloud(16384, 2024), 4)


# ---- 1. operand maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap", [0, 6, 14])
@pytest.mark.parametrize("sliced", [False, True], ids=["one-slice", "sliced"])
def test_selection_weight_is_an_exact_copy(dev, S, axis_cloud, sliced, tap):
    cin, cout, K = 37, 21, 15
    idx = axis_cloud if sliced else _axis_rows(9000, 5)
    n = len(idx)
    fs, xs = _slices(S, n, cin, cout, K)
    assert (fs > 1 and xs > 1) if sliced else (fs, xs) == (1, 1), (n, fs, xs)
    rng = np.random.default_rng(tap + 100 * sliced)
    x = rng.normal(size=(n, cin)).astype(np.float32)
    dy = rng.normal(size=(n, cout)).astype(np.float32)
    sel = (3 * np.arange(cout) + 1) % cin                      # output o reads input channel sel[o]; injective
    assert len(set(sel)) == cout and not np.array_equal(sel, np.arange(cout))
    w = np.zeros((cout, K, cin), np.float32)
    w[np.arange(cout), tap, sel] = 1.0
    with engine("mfma"):
        y, dx, _, _ = V._run(dev, idx, AXIS_SHAPE, 2, x, w.reshape((cout,) + AXIS_KSIZE + (cin,)), None, AXIS_KSIZE,
                             AXIS_DIL, dy)
    nbr = R.neighbours(idx, AXIS_SHAPE, AXIS_KSIZE, AXIS_DIL)
    has = nbr[:, tap] >= 0
    assert has.sum() > 20
    want = np.where(has[:, None], x[np.maximum(nbr[:, tap], 0)][:, sel], 0.0).astype(np.float32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), "forward, tap %d" % tap
    want_dx = np.zeros((n, cin), np.float32)
    rows = np.nonzero(has)[0]
    want_dx[nbr[rows, tap][:, None], sel[None, :]] = dy[rows]   # distinct voxels: one source row per target at most
    assert np.array_equal(dx.view(np.uint32), want_dx.view(np.uint32)), "dX, tap %d" % tap


# ---- 2. equality with the VALU engine where the plan has one slice -------------------------------------------------
def _both_engines(dev, coords, extent, cin, cout, seed):
    n = len(coords)
    idx = R.with_batch(coords, np.zeros(n))
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, cin)).astype(np.float32)
    w = (rng.normal(size=(cout, 3, 3, 3, cin)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.normal(size=cout).astype(np.float32)
    dy = rng.normal(size=(n, cout)).astype(np.float32)
    out = {}
    for name in ("valu", "mfma"):
        with engine(name):
            out[name] = V._run(dev, idx, [extent] * 3, 1, x, w, b, (3, 3, 3), (1, 1, 1), dy)
    return out, (idx, x, w, b, dy)


EQUAL_SHAPES = [("small", 8200, 0, 6, 5, "TILE_32X32"), ("wide", 5500, 0, 136, 200, "TILE_64X64"),
                ("wide-duplicates", 5500, 550, 136, 200, "TILE_64X64"), ("tall", 32805, 0, 20, 24, "TILE_128X32"),
                ("tall-duplicates", 32805, 300, 20, 24, "TILE_128X32")]


@pytest.mark.parametrize("name,rows,repeats,cin,cout,tile", EQUAL_SHAPES, ids=[s[0] for s in EQUAL_SHAPES])
def test_one_slice_equals_the_valu_engine(dev, S, name, rows, repeats, cin, cout, tile):
    extent = 160 if rows > 6000 else 80
    coords = R.shell_cloud(rows, 2025 if rows > 6000 else 2026, extent=extent)
    if repeats:
        coords = V._with_repeats(coords, repeats, 1)
    n = len(coords)
    plan = S.subm_engine_plan(S.ENGINE_MFMA, n, cin, cout, 27)
    assert plan[0] == plan[1] == getattr(S, tile) and plan[5:] == (1, 1), plan
    out, _ = _both_engines(dev, coords, extent, cin, cout, rows + repeats)
    for q, what in ((0, "y"), (1, "dX")):
        a, b = out["valu"][q], out["mfma"][q]
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        print("%s %s: largest |mfma - valu| = %.3g" % (name, what, float(diff.max())))
        assert np.array_equal(a, b), "%s %s: %d values differ from the VALU engine, largest difference %g" % (
            name, what, int((a != b).sum()), float(diff.max()))
    for q in (2, 3):                                            # dW and dB are the same kernels on the same inputs
        assert np.array_equal(out["valu"][q].view(np.uint32), out["mfma"][q].view(np.uint32))


def test_the_300_row_shape_is_sliced_and_meets_the_float64_bar(dev, S):
    n, cin, cout = 300, 6, 5
    assert S.subm_plan(n, cin, cout, 27)[:2] == (S.TILE_32X32, S.TILE_32X32)
    fs, xs = _slices(S, n, cin, cout, 27)
    assert fs > 1 and xs > 1
    coords = R.shell_cloud(n, n + cin, extent=48)
    idx = R.with_batch(coords, np.random.default_rng(n).integers(0, 2, n))
    with engine("mfma"):
        V._check_case(dev, idx, [48] * 3, 2, cin, cout, 3, seed=cin, what="mfma, 300 rows 6->5")


# ---- 3. sliced shapes against float64 -------------------------------------------------------------------------------
def test_sliced_stage_4_and_stage_3(dev, S, shell):
    for stage, c, rows in ((4, 512, 73), (3, 256, 271)):
        coords = shell[stage]
        assert len(coords) == rows
        fs, xs = _slices(S, rows, c, c, 27)
        assert fs > 1 and xs > 1
        idx = R.with_batch(coords, np.zeros(rows))
        with engine("mfma"):
            V._check_case(dev, idx, (coords.max(0) + 3).tolist(), 1, c, c, 3, seed=c, what="mfma stage %d" % stage)


def test_sliced_partial_tiles_at_40_to_52(dev, S, shell):
    """Nothing is a multiple of 16 or 32: 73 rows (a partial row tile), 40 and 52 channels (partial slices and column tiles)."""
    coords = shell[4]
    fs, xs = _slices(S, 73, 40, 52, 27)
    assert fs > 1 and xs > 1
    with engine("mfma"):
        V._check_case(dev, R.with_batch(coords, np.zeros(73)), (coords.max(0) + 3).tolist(), 1, 40, 52, 3, seed=4052,
                      what="mfma 73 rows 40->52")


@pytest.mark.parametrize("rows", [None, 2300], ids=["axis-cloud", "ragged-last-slice"])
def test_sliced_fifteen_taps(dev, S, axis_cloud, rows):
    """K = 15 on the (3, 1, 5) / dilation (1, 2, 3) geometry.  The whole cloud (2 469 rows, 78 tiles) runs in 5 slices of 3
    taps; its first 2 300 rows (72 tiles) in 8 slices, the last of ONE tap where the others have two: the clamp of a
    slice's last tap to K."""
    idx = axis_cloud if rows is None else axis_cloud[:rows]
    fs, xs = _slices(S, len(idx), 5, 7, 15)
    assert fs > 1 and xs > 1, (fs, xs)
    if rows is not None:
        assert 15 % fs != 0 and 15 % xs != 0, "the slices divide K: no slice is cut short any more (%d, %d)" % (fs, xs)
    with engine("mfma"):
        _, nbr = V._check_case(dev, idx, AXIS_SHAPE, 2, 5, 7, AXIS_KSIZE, AXIS_DIL, seed=9, what="mfma K = 15")
    assert ((nbr >= 0).sum(0) > 20).all()


def _repeated_cloud():
    coords = V._with_repeats(R.shell_cloud(900, 12, extent=48), 60, 12)
    return R.with_batch(coords, np.zeros(len(coords)))


def test_sliced_dx_with_the_row_mask_in_the_epilogue(dev, S):
    idx = _repeated_cloud()
    fs, xs = _slices(S, len(idx), 24, 40, 27)
    assert len(idx) == 960 and fs > 1 and xs > 1
    with engine("mfma"):
        y, nbr = V._check_case(dev, idx, [48] * 3, 1, 24, 40, 3, seed=2440, what="mfma, 60 repeated rows")
    V._rows_of_one_voxel_agree(y, nbr, idx, [48] * 3, 50)


# ---- 4. determinism and workspace independence, through the C ABI ------------------------------------------------
def test_workspace_contents_and_stream_do_not_change_a_bit(dev, S, shell):
    from gaussiancity_amd import sparse as SP
    coords, c, K = shell[4], 512, 27
    n = len(coords)
    fs, xs = _slices(S, n, c, c, K)
    assert fs > 1 and xs > 1
    fwd_bytes, bwd_bytes = S.subm_engine_workspace_bytes(S.ENGINE_MFMA, n, c, c, K, 0)
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(n, c, generator=g).to(dev), torch.randn(n, c, generator=g).to(dev)
    w = (torch.randn(c, K, c, generator=g) / (K * c) ** 0.5).to(dev)
    b = torch.randn(c, generator=g).to(dev)
    idx = torch.from_numpy(R.with_batch(coords, np.zeros(n))).to(dev)
    rb = SP.Rulebook(idx, (coords.max(0) + 3).tolist(), 1, (3, 3, 3), (1, 1, 1))
    assert rb.dups == 0
    L = S.lib()
    second = torch.cuda.Stream(device=dev)
    results = []
    for fill, stream in ((0xFF, None), (0x00, None), (0xFF, second)):
        ws_f = torch.full((fwd_bytes,), fill, dtype=torch.uint8, device=dev)
        ws_b = torch.full((bwd_bytes,), fill, dtype=torch.uint8, device=dev)
        y, dx = torch.full((n, c), 7.0, device=dev), torch.full((n, c), 7.0, device=dev)
        torch.cuda.synchronize()
        st = C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        S.check(L.gcs_subm_forward_engine(S.ENGINE_MFMA, rb.buf.data_ptr(), n, K, x.data_ptr(), c, w.data_ptr(),
                                          b.data_ptr(), c, y.data_ptr(), ws_f.data_ptr(), fwd_bytes, st), "forward")
        S.check(L.gcs_subm_backward_engine(S.ENGINE_MFMA, rb.buf.data_ptr(), n, K, 0, x.data_ptr(), c, w.data_ptr(), c,
                                           dy.data_ptr(), dx.data_ptr(), None, None, ws_b.data_ptr(), bwd_bytes, st),
                "backward")
        torch.cuda.synchronize()
        results.append((y.cpu().numpy(), dx.cpu().numpy()))
    for y, dx in results:
        assert np.isfinite(y).all() and np.isfinite(dx).all()
    for y, dx in results[1:]:
        assert np.array_equal(y.view(np.uint32), results[0][0].view(np.uint32)), "forward depends on workspace or stream"
        assert np.array_equal(dx.view(np.uint32), results[0][1].view(np.uint32)), "dX depends on workspace or stream"
    nbr = R.neighbours(idx.cpu().numpy(), (coords.max(0) + 3).tolist(), (3, 3, 3), (1, 1, 1))
    wn = w.cpu().numpy().reshape(c, 3, 3, 3, c)
    ry, sy = R.conv_forward(x.cpu().numpy(), wn, b.cpu().numpy(), nbr)
    V._close(results[0][0], ry, sy, "C ABI forward")


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------
def test_an_empty_cloud(dev):
    idx = np.zeros((0, 4), np.int32)
    with engine("mfma"):
        V._check_case(dev, idx, [5, 6, 7], 2, 4, 3, 3, seed=0, what="mfma n = 0")


@pytest.mark.parametrize("grads", [g for g in itertools.product((True, False), repeat=3) if any(g)],
                         ids=lambda g: "".join(n for n, on in zip(("dx", "dw", "db"), g) if on))
def test_every_subset_of_gradients(dev, grads):
    with engine("mfma"):
        V._check_case(dev, _repeated_cloud(), [48] * 3, 1, 24, 40, 3, seed=12, what="mfma grads %r" % (grads,), grads=grads)


def test_a_layers_backward_runs_its_forwards_engine(dev, S, shell):
    import spconv.pytorch as spconv
    from gaussiancity_amd import sparse as SP
    coords, c = shell[3], 256
    n = len(coords)
    assert _slices(S, n, c, c, 27)[1] > 1
    conv = spconv.SubMConv3d(c, c, 3).to(dev)
    g = torch.Generator().manual_seed(3)
    x0, dy = torch.randn(n, c, generator=g).to(dev), torch.randn(n, c, generator=g).to(dev)
    idx = torch.from_numpy(R.with_batch(coords, np.zeros(n))).to(dev)
    shape = (coords.max(0) + 3).tolist()

    def run(forward_engine, backward_engine):
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        with engine(forward_engine):
            y = conv(spconv.SparseConvTensor(x, idx, shape, 1)).features
        with engine(backward_engine):
            y.backward(dy)
        return y.detach().cpu().numpy(), x.grad.cpu().numpy()

    start = SP.get_engine()
    SP.reset_stats()
    y_m, dx_m = run("mfma", "mfma")
    y_v, dx_v = run("valu", "valu")
    assert (SP.stats()["conv_forward_calls_mfma"], SP.stats()["conv_forward_calls_valu"]) == (1, 1)
    y_s, dx_s = run("mfma", "valu")
    assert (SP.stats()["conv_forward_calls_mfma"], SP.stats()["conv_forward_calls_valu"]) == (2, 1)
    assert SP.get_engine() == start
    assert np.array_equal(y_s.view(np.uint32), y_m.view(np.uint32))
    assert np.array_equal(dx_s.view(np.uint32), dx_m.view(np.uint32)), "the backward did not run the forward's engine"
    assert not np.array_equal(dx_m, dx_v), "sliced sums and one chain gave the same bits: the comparison shows nothing"
    y_s, dx_s = run("valu", "mfma")
    assert np.array_equal(dx_s.view(np.uint32), dx_v.view(np.uint32)) and np.array_equal(y_s.view(np.uint32), y_v.view(np.uint32))


def test_two_engines_share_one_rulebook(dev):
    import spconv.pytorch as spconv
    from gaussiancity_amd import sparse as SP
    coords = R.shell_cloud(2000, 3, extent=50)
    idx_np = R.with_batch(coords, np.zeros(len(coords)))
    x = np.random.default_rng(8).normal(size=(len(coords), 8)).astype(np.float32)
    t = spconv.SparseConvTensor(torch.from_numpy(x).to(dev), torch.from_numpy(idx_np).to(dev), [50, 50, 50], 1)
    a = spconv.SubMConv3d(8, 8, 3, indice_key="s0").to(dev)
    b = spconv.SubMConv3d(8, 8, 3, indice_key="s0").to(dev)
    SP.reset_stats()
    with engine("valu"):
        ya = a(t)
    with engine("mfma"):
        yb = b(t)
    st = SP.stats()
    assert (st["rulebook_builds"], st["conv_forward_calls_valu"], st["conv_forward_calls_mfma"]) == (1, 1, 1)
    assert yb.indice_dict is t.indice_dict and ya.indice_dict is t.indice_dict
    nbr = R.neighbours(idx_np, [50] * 3, (3, 3, 3), (1, 1, 1))
    for conv, out in ((a, ya), (b, yb)):
        ry, sy = R.conv_forward(x, conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), nbr)
        V._close(out.features.detach().cpu().numpy(), ry, sy, "shared rulebook")
