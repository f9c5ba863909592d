"""-m gpu: the weight gradient of the matrix-core engine (k_subm_dw_mfma, gaussiancity_amd/csrc/gcs_mfma.h, DESIGN.md
section 15) against exact integer sums, the VALU engine's k_subm_dw and the float64 reference tests/sparse_ref.py.

k_subm_dw builds every element of a slice's partial as one fmaf chain from 0.0f over the slice's pairs in list order,
and the f32-input MFMA is a k-ordered fmaf chain, so under the same tile, the same pair slices and the same zero-padded
last chunk the two engines' dW are the same BITS at every shape: that is what is asserted, not a tolerance.

Every test first asserts that the engine says it runs dW on the matrix cores (gcs_engine_products), so that none of them
passes on a library whose engine still launches k_subm_dw, and then the dW tile and slice count of its shape
(gcs_subm_engine_plan), so that a moved threshold fails loudly instead of un-covering a path.

SHAPES (test_sparse_dw_engine_host.py asserts the same plan without a GPU):

  name           rows   Cin->Cout  kernel  dW tile  slices  what it can catch
  tiny            300     6->5     3       32 x 32  1       direct store to dw, ragged tile both ways, last chunk < 16 pairs
  ragged-slices  2300    20->24    3       32 x 32  8       partials + k_sum_slices, ragged last slice
  wide           1500   136->200   3       64 x 64  5       2 x 2 accumulators, 12 tiles with an 8-wide remainder on both sides
  wide-one        300    64->64    3       64 x 64  1       64 x 64 direct store
  stem            600   128->32    5       32 x 32  2       K = 125 taps, four column tiles
  k1              300    16->16    1       32 x 32  1       a single tap
  axis           2000    20->24    3       32 x 32  7       points on one line: 24 of 27 taps have no pair, their block must be zeros
  duplicates     1500    20->24    3       32 x 32  5       every voxel 1 to 3 times: pair lists over all rows, representatives as neighbours

Bars: exact where stated; otherwise the project's |got - ref| <= 1e-5 * sum |terms| (test_sparse_variants_gpu.py).

The module's name puts it after the rasteriser's GPU modules, as test_varlen_attention_gpu.py explains."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sparse_ref as R
import test_sparse_variants_gpu as V

pytestmark = pytest.mark.gpu

# name: (rows, cin, cout, kernel size, dW tile, dW slices)
SHAPES = {
    "tiny": (300, 6, 5, 3, "TILE_32X32", 1),
    "ragged-slices": (2300, 20, 24, 3, "TILE_32X32", 8),
    "wide": (1500, 136, 200, 3, "TILE_64X64", 5),
    "wide-one": (300, 64, 64, 3, "TILE_64X64", 1),
    "stem": (600, 128, 32, 5, "TILE_32X32", 2),
    "k1": (300, 16, 16, 1, "TILE_32X32", 1),
    "axis": (2000, 20, 24, 3, "TILE_32X32", 7),
    "duplicates": (1500, 20, 24, 3, "TILE_32X32", 5),
}
AXIS_LENGTH = 2600


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(indices [rows, 4] int32, spatial shape, batch size) of a shape of the table; the same arrays for every test."""
    rows = SHAPES[name][0]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "axis":                                         # one line along the last axis, rows shuffled
        z = rng.permutation(AXIS_LENGTH)[:rows]
        coords = np.stack([np.ones(rows, np.int64), np.ones(rows, np.int64), z], 1)
        return R.with_batch(coords, np.zeros(rows)), (3, 3, AXIS_LENGTH), 1
    if name == "duplicates":
        base = R.shell_cloud(800, 31, extent=48)
        coords = np.repeat(base, rng.integers(1, 4, len(base)), axis=0)
        assert len(coords) >= rows
        coords = coords[rng.permutation(len(coords))][:rows]
        return R.with_batch(coords, np.zeros(rows)), (48, 48, 48), 1
    extent = 64 if rows > 2000 else 48
    coords = R.shell_cloud(rows, rows + SHAPES[name][1], extent=extent)
    return R.with_batch(coords, rng.integers(0, 2, rows)), (extent,) * 3, 2


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Random x, w, dy of a shape and its neighbour map; shared and never written."""
    rows, cin, cout, k = SHAPES[name][:4]
    idx, shape, _ = cloud(name)
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    x = rng.normal(size=(rows, cin)).astype(np.float32)
    w = (rng.normal(size=(cout, k, k, k, cin)) / np.sqrt(cin * k ** 3)).astype(np.float32)
    dy = rng.normal(size=(rows, cout)).astype(np.float32)
    nbr = R.neighbours(idx, shape, (k,) * 3, (1, 1, 1))
    return x, w, dy, nbr


@functools.lru_cache(maxsize=None)
def reference(name):
    """((dx, scale), (dw, scale), (db, scale)) of tests/sparse_ref.py in float64, computed once per shape."""
    x, w, dy, nbr = inputs(name)
    return R.conv_backward(x, w, nbr, dy)


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


@pytest.fixture(scope="module")
def rulebooks(dev):
    """name -> Rulebook, built on first use and shared by the module's tests."""
    from gaussiancity_amd import sparse as SP
    built = {}

    def get(name):
        if name not in built:
            idx, shape, batch = cloud(name)
            k = SHAPES[name][3]
            built[name] = SP.Rulebook(torch.from_numpy(idx).to(dev), shape, batch, (k,) * 3, (1, 1, 1))
        return built[name]

    return get


@contextlib.contextmanager
def engine(name):
    from gaussiancity_amd import sparse as SP
    prev = SP.set_engine(name)
    try:
        yield
    finally:
        SP.set_engine(prev)


def _enter(S, name):
    """What every test starts with: the engine runs dW on the matrix cores, and the shape still has its tile and slices."""
    from gaussiancity_amd import sparse as SP
    assert "dw" in SP.engine_products("mfma"), "the matrix-core engine does not run dW"
    rows, cin, cout, k, tile, slices = SHAPES[name]
    assert len(cloud(name)[0]) == rows
    for eng in (S.ENGINE_VALU, S.ENGINE_MFMA):
        plan = S.subm_engine_plan(eng, rows, cin, cout, k ** 3)
        assert (plan[2], plan[3]) == (getattr(S, tile), slices), "%s: dW plan moved to %r" % (name, plan[2:4])
    return rows, cin, cout, k ** 3


def _backward(S, dev, rb, eng, x, w, dy, cin, cout, want_dx=False, want_db=False, fill=0x00, stream=None):
    """gcs_subm_backward_engine through the C ABI on device tensors; dw (and dx, db when asked for) as numpy.  The
    outputs are NaN before the call and the workspace holds `fill` in every byte."""
    n, K = rb.n, rb.kvol
    ws_bytes = S.subm_engine_workspace_bytes(eng, n, cin, cout, K, rb.dups)[1]
    ws = torch.full((max(ws_bytes, 1),), fill, dtype=torch.uint8, device=dev)
    nan = float("nan")
    dw = torch.full((cout, K, cin), nan, device=dev)
    dx = torch.full((n, cin), nan, device=dev) if want_dx else None
    db = torch.full((cout,), nan, device=dev) if want_db else None
    ptr = lambda t: t.data_ptr() if (t is not None and t.numel()) else None  # noqa: E731
    torch.cuda.synchronize()
    st = C.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    S.check(S.lib().gcs_subm_backward_engine(eng, rb.buf.data_ptr(), n, K, rb.dups, ptr(x), cin, w.data_ptr(), cout,
                                             ptr(dy), ptr(dx), dw.data_ptr(), ptr(db), ws.data_ptr(), ws_bytes, st),
            "gcs_subm_backward_engine")
    torch.cuda.synchronize()
    out = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return out(dw), out(dx), out(db)


def _device_inputs(dev, name):
    x, w, dy, _ = inputs(name)
    cout, cin = w.shape[0], w.shape[-1]
    return (torch.from_numpy(x).to(dev), torch.from_numpy(w.reshape(cout, -1, cin)).to(dev).contiguous(),
            torch.from_numpy(dy).to(dev))


def _same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- 1. the operand maps, exactly ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "wide", "stem"])
def test_integer_inputs_give_the_exact_integer_sums(dev, S, rulebooks, name):
    """X holds integers in [-4, 4]; dY is zero except in one column o*, which holds integer row weights.  Then
    dW[o*][k][c] = sum over the pairs (i, j) of tap k of weight_i * X[j][c], an integer far below 2^24, and every other
    output row is zero.  Cin != Cout, so a transposed tile or a swapped row / column of the C/D store cannot pass; o* is
    taken in the first tile and in the ragged last one."""
    n, cin, cout, K = _enter(S, name)
    assert cin != cout
    rb = rulebooks(name)
    nbr = inputs(name)[3]
    rng = np.random.default_rng(n + cin)
    xi = rng.integers(-4, 5, (n, cin))
    w = torch.zeros((cout, K, cin), device=dev)
    for o_star in (1, cout - 2):
        wi = rng.integers(-3, 4, n)
        dyi = np.zeros((n, cout), np.int64)
        dyi[:, o_star] = wi
        want = np.zeros((cout, K, cin), np.int64)
        for k in range(K):
            i = np.nonzero(nbr[:, k] >= 0)[0]
            want[o_star, k] = wi[i] @ xi[nbr[i, k]]
        assert np.abs(want).max() < 2 ** 24 and np.count_nonzero(want[o_star]) > K * cin // 2
        dw, _, _ = _backward(S, dev, rb, S.ENGINE_MFMA, torch.from_numpy(xi.astype(np.float32)).to(dev), w,
                             torch.from_numpy(dyi.astype(np.float32)).to(dev), cin, cout)
        rest = np.delete(dw, o_star, axis=0)
        assert np.array_equal(rest, np.zeros_like(rest)), "%s: rows other than o* = %d are not zero" % (name, o_star)
        assert np.array_equal(dw[o_star], want[o_star].astype(np.float32)), "%s: dW[o* = %d] is not the integer sum" % (
            name, o_star)


# ---- 2. the VALU engine's bits, at every shape -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_dw_has_the_valu_engines_bits(dev, S, rulebooks, name):
    n, cin, cout, K = _enter(S, name)
    rb = rulebooks(name)
    pairs = np.array(rb.pairs)
    slices = SHAPES[name][5]
    if name == "axis":
        assert (pairs > 0).sum() == 3 and pairs[K // 2] == n, "the cloud is no longer a line"
    if name == "duplicates":
        assert rb.dups == 1
    if name == "tiny":
        assert (pairs % 16 != 0).any(), "no tap's last chunk is cut short"
    if name == "ragged-slices":
        assert (pairs % slices != 0).any(), "every tap's pairs divide into equal slices"
    x, w, dy = _device_inputs(dev, name)
    dw_v, _, _ = _backward(S, dev, rb, S.ENGINE_VALU, x, w, dy, cin, cout, True, True)
    dw_m, dx_m, db_m = _backward(S, dev, rb, S.ENGINE_MFMA, x, w, dy, cin, cout, True, True)
    assert np.isfinite(dw_v).all() and np.abs(dw_v).max() > 0
    diff = np.abs(dw_m.astype(np.float64) - dw_v.astype(np.float64))
    print("%s dW: largest |mfma - valu| = %.3g" % (name, float(np.nanmax(diff))))
    assert _same_bits(dw_m, dw_v), "%s: %d of %d dW values differ from the VALU engine's" % (
        name, int((dw_m.view(np.int32) != dw_v.view(np.int32)).sum()), dw_v.size)
    if name == "axis":
        empty = np.nonzero(pairs == 0)[0]
        assert len(empty) == 24 and _same_bits(dw_m[:, empty], np.zeros_like(dw_m[:, empty]))
    (rdx, sdx), _, (rdb, sdb) = reference(name)
    V._close(dx_m, rdx, sdx, name + " dX")
    V._close(db_m, rdb, sdb, name + " dB")


# ---- 3. the float64 bar -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged-slices", "wide", "duplicates"])
def test_dw_meets_the_float64_bar(dev, S, rulebooks, name):
    n, cin, cout, K = _enter(S, name)
    x, w, dy = _device_inputs(dev, name)
    dw, _, _ = _backward(S, dev, rulebooks(name), S.ENGINE_MFMA, x, w, dy, cin, cout)
    _, (rdw, sdw), _ = reference(name)
    V._close(dw.reshape(rdw.shape), rdw, sdw, name + " dW")


# ---- 4. workspace contents, stream, repetition -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged-slices", "wide", "wide-one"])
def test_workspace_contents_stream_and_repetition_do_not_change_a_bit(dev, S, rulebooks, name):
    """dw is NaN before every call (_backward), so every element must be written; a workspace of 0xFF bytes is NaN in
    every float of the partials."""
    n, cin, cout, K = _enter(S, name)
    rb = rulebooks(name)
    x, w, dy = _device_inputs(dev, name)
    first, _, _ = _backward(S, dev, rb, S.ENGINE_MFMA, x, w, dy, cin, cout)
    assert np.isfinite(first).all(), "%d elements of dW were not written" % int((~np.isfinite(first)).sum())
    again, _, _ = _backward(S, dev, rb, S.ENGINE_MFMA, x, w, dy, cin, cout)
    assert _same_bits(again, first), "two consecutive runs differ"
    filled, _, _ = _backward(S, dev, rb, S.ENGINE_MFMA, x, w, dy, cin, cout, fill=0xFF)
    assert _same_bits(filled, first), "dW depends on what the workspace held"
    other, _, _ = _backward(S, dev, rb, S.ENGINE_MFMA, x, w, dy, cin, cout, fill=0xFF,
                            stream=torch.cuda.Stream(device=dev))
    assert _same_bits(other, first), "dW depends on the stream"


# ---- 5. through the module ---------------------------------------------------------------------------------------------
def test_the_module_counts_and_runs_the_engines_dw(dev, S):
    import spconv.pytorch as spconv
    from gaussiancity_amd import sparse as SP
    name = "ragged-slices"
    n, cin, cout, K = _enter(S, name)
    idx, shape, batch = cloud(name)
    x_np, _, dy_np, _ = inputs(name)
    conv = spconv.SubMConv3d(cin, cout, 3).to(dev)
    idx_t, dy = torch.from_numpy(idx).to(dev), torch.from_numpy(dy_np).to(dev)

    def run(engine_name, weight_grad=True):
        conv.zero_grad()
        conv.weight.requires_grad_(weight_grad)
        x = torch.from_numpy(x_np).to(dev).requires_grad_(True)
        with engine(engine_name):
            conv(spconv.SparseConvTensor(x, idx_t, list(shape), batch)).features.backward(dy)
        grad = conv.weight.grad
        return None if grad is None else grad.cpu().numpy(), x.grad.cpu().numpy()

    counts = lambda: (SP.stats()["conv_dw_calls_valu"], SP.stats()["conv_dw_calls_mfma"])  # noqa: E731
    v0, m0 = counts()
    dw_m, dx_m = run("mfma")
    assert counts() == (v0, m0 + 1)
    dw_v, _ = run("valu")
    assert counts() == (v0 + 1, m0 + 1)
    assert dw_m.shape == (cout, 3, 3, 3, cin) and np.abs(dw_v).max() > 0
    assert _same_bits(dw_m, dw_v), "weight.grad under \"mfma\" is not the \"valu\" run's"
    none, dx_only = run("mfma", weight_grad=False)
    assert counts() == (v0 + 1, m0 + 1), "a backward without the weight gradient was counted"
    assert none is None and _same_bits(dx_only, dx_m), "dX alone differs from dX next to dW"
    conv.weight.requires_grad_(True)


# ---- 6. the empty cloud ------------------------------------------------------------------------------------------------
def test_an_empty_cloud_clears_dw(dev, S):
    from gaussiancity_amd import sparse as SP
    assert "dw" in SP.engine_products("mfma")
    cin, cout, K = 20, 24, 27
    rb = SP.Rulebook(torch.zeros((0, 4), dtype=torch.int32, device=dev), (5, 6, 7), 2, (3, 3, 3), (1, 1, 1))
    x, dy = torch.zeros((0, cin), device=dev), torch.zeros((0, cout), device=dev)
    w = torch.ones((cout, K, cin), device=dev)
    dw, _, db = _backward(S, dev, rb, S.ENGINE_MFMA, x, w, dy, cin, cout, want_db=True, fill=0xFF)
    assert _same_bits(dw, np.zeros_like(dw)) and _same_bits(db, np.zeros_like(db))
