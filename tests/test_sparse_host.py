"""CPU tests of the sparse operators (libgcs_hip.so, include/gcs.h; gaussiancity_amd.sparse; the spconv and
torch_scatter drop-ins): the library loads (tests/test_cabi.py holds its exports to the header), the ABI rejects bad
arguments before it touches the device, the drop-in modules import and construct as spconv's do, and the float64
reference (tests/sparse_ref.py) agrees with torch's dense conv3d."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_ref as R


@pytest.fixture(scope="module")
def lib():
    from gaussiancity_amd import _native_s as S
    return S.lib()


def test_workspace_queries(lib):
    # the neighbour map alone is N * K int32
    assert lib.gcs_subm_rulebook_bytes(16384, 125) >= 16384 * 125 * 4
    assert lib.gcs_subm_rulebook_scratch_bytes(16384) >= 2 * 16384 * 12
    base = lib.gcs_subm_backward_workspace_bytes(1000, 32, 32, 27, 0)
    assert lib.gcs_subm_backward_workspace_bytes(1000, 32, 32, 27, 1) >= base + 1000 * 32 * 4   # the fold of dy
    assert lib.gcs_subm_rulebook_bytes(-1, 27) == 0 and b"n out of range" in lib.gcs_last_error()
    assert lib.gcs_subm_rulebook_bytes(10, 0) == 0


def test_plan_names_the_kernels_of_ptv3s_own_sizes(lib):
    """gcs_subm_plan is the chooser the launches dispatch from; the GPU tests assert it before they run a variant."""
    from gaussiancity_amd import _native_s as S
    # stage 0 of the inference loop, 518 k points: the stem forward, the 32 -> 32 layers forward and their dX take
    # the 128 x 32 tile; the stem's dX has 128 output columns and takes the 64 x 64 one
    fwd, dx, dw, dws, dbs = S.subm_plan(518000, 128, 32, 125)
    assert (fwd, dx, dw) == (S.TILE_128X32, S.TILE_64X64, S.TILE_32X32) and 1 < dws <= 32 and dbs == 64
    assert S.subm_plan(518000, 32, 32, 27)[:3] == (S.TILE_128X32, S.TILE_128X32, S.TILE_32X32)
    # the thresholds: 256 workgroups of 128 rows, or of 64 x 64; at most 16 or more than 32 columns leave the tall tile
    assert S.subm_plan(32640, 32, 32, 27)[:2] == (S.TILE_32X32, S.TILE_32X32)
    assert S.subm_plan(32641, 32, 17, 27)[:2] == (S.TILE_128X32, S.TILE_128X32)
    assert S.subm_plan(32641, 16, 33, 27)[:2] == (S.TILE_64X64, S.TILE_32X32)
    assert S.subm_plan(16320, 64, 64, 27)[:2] == (S.TILE_32X32, S.TILE_32X32)
    assert S.subm_plan(16321, 64, 64, 27)[:3] == (S.TILE_64X64, S.TILE_64X64, S.TILE_64X64)
    assert S.subm_plan(4033, 256, 200, 27)[:3] == (S.TILE_64X64, S.TILE_64X64, S.TILE_64X64)
    # dW: 64 x 64 only when both channel counts reach 64; slices: ceil(2048 / workgroups), at least 256 rows each, 32 at most
    assert S.subm_plan(5000, 64, 63, 27)[2] == S.TILE_32X32 and S.subm_plan(5000, 64, 64, 27)[2] == S.TILE_64X64
    assert S.subm_plan(511, 64, 64, 27)[3] == 1 and S.subm_plan(5000, 64, 64, 27)[3] == 19
    assert S.subm_plan(16384, 512, 512, 27)[3] == 2 and S.subm_plan(10 ** 6, 4, 4, 27)[3] == 32
    # dB: one slice per 2048 rows, 64 at most
    assert [S.subm_plan(n, 4, 4, 27)[4] for n in (0, 4095, 4096, 10 ** 6)] == [1, 1, 2, 64]
    # the workspace follows the same plan: the dW slices and the dB slices are in it
    n, cin, cout, k = 5000, 64, 64, 27
    assert lib.gcs_subm_backward_workspace_bytes(n, cin, cout, k, 0) >= 19 * cout * k * cin * 4 + 2 * cout * 4


def test_plan_rejects_bad_arguments(lib):
    out = (C.c_int32 * 5)()
    assert lib.gcs_subm_plan(-1, 4, 4, 27, out) < 0 and b"n out of range" in lib.gcs_last_error()
    assert lib.gcs_subm_plan(2 ** 31, 4, 4, 27, out) < 0
    assert lib.gcs_subm_plan(10, 0, 4, 27, out) < 0 and b"channel" in lib.gcs_last_error()
    assert lib.gcs_subm_plan(10, 4, 65537, 27, out) < 0 and b"channel" in lib.gcs_last_error()
    assert lib.gcs_subm_plan(10, 4, 4, 0, out) < 0 and b"kernel volume" in lib.gcs_last_error()
    assert lib.gcs_subm_plan(10, 4, 4, 1025, out) < 0
    assert lib.gcs_subm_plan(2 ** 30, 4, 4, 27, out) < 0 and b"kernel volume" in lib.gcs_last_error()   # n * K beyond int32
    assert lib.gcs_subm_plan(10, 4, 4, 27, None) < 0 and b"null plan" in lib.gcs_last_error()
    assert lib.gcs_subm_plan(0, 1, 1, 1, out) == 0 and list(out) == [0, 0, 0, 1, 1]


def _rulebook(lib, ksize=(3, 3, 3), dilation=(1, 1, 1), shape=(8, 8, 8), batch=1, n=4, buf=1, scratch=1, size=1 << 20):
    from gaussiancity_amd import _native_s as S
    info = (C.c_int32 * 200)()
    return lib.gcs_subm_rulebook(1, n, batch, S.triple(shape), S.triple(ksize), S.triple(dilation), buf, size, scratch,
                                 size, info, None)


def test_rulebook_rejects_bad_arguments_before_touching_the_device(lib):
    # dummy non-null device addresses: every call below must fail in the argument checks
    assert _rulebook(lib, ksize=(3, 4, 3)) < 0 and b"odd" in lib.gcs_last_error()
    assert _rulebook(lib, ksize=(0, 3, 3)) < 0
    assert _rulebook(lib, dilation=(1, 0, 1)) < 0 and b"dilation" in lib.gcs_last_error()
    assert _rulebook(lib, shape=(8, 0, 8)) < 0
    assert _rulebook(lib, batch=0) < 0
    big = 2 ** 31 - 1
    assert _rulebook(lib, shape=(big, big, big), batch=4) < 0 and b"64-bit key" in lib.gcs_last_error()
    assert _rulebook(lib, buf=None) < 0 and b"rulebook buffer" in lib.gcs_last_error()
    assert _rulebook(lib, scratch=None) < 0 and b"scratch" in lib.gcs_last_error()
    assert _rulebook(lib, size=16) < 0
    assert lib.gcs_subm_rulebook(None, 4, 1, None, None, None, 1, 1 << 20, 1, 1 << 20, None, None) < 0


def test_convolution_and_segment_entry_points_reject_bad_arguments(lib):
    assert lib.gcs_subm_forward(None, 10, 27, 1, 4, 1, None, 4, 1, None) < 0 and b"null" in lib.gcs_last_error()
    assert lib.gcs_subm_forward(1, 10, 27, None, 4, 1, None, 4, 1, None) < 0
    assert lib.gcs_subm_forward(1, 10, 27, 1, 0, 1, None, 4, 1, None) < 0 and b"channel" in lib.gcs_last_error()
    assert lib.gcs_subm_forward(1, 10, 2000, 1, 4, 1, None, 4, 1, None) < 0
    assert lib.gcs_subm_backward(1, 10, 27, 0, 1, 4, 1, 4, 1, 1, 1, 1, None, 0, None) < 0
    assert b"workspace" in lib.gcs_last_error()
    ws = lib.gcs_subm_backward_workspace_bytes(10, 4, 4, 27, 0)
    assert lib.gcs_subm_backward(1, 10, 27, 0, 1, 4, 1, 4, None, 1, None, None, 1, ws, None) < 0
    assert lib.gcs_segment_csr_forward(1, 10, 3, 1, 4, 7, 1, None, None) < 0 and b"reduce" in lib.gcs_last_error()
    assert lib.gcs_segment_csr_forward(1, 10, 3, None, 4, 0, 1, None, None) < 0
    assert lib.gcs_segment_csr_forward(1, 10, 3, 1, 4, 3, 1, None, None) < 0 and b"arg" in lib.gcs_last_error()
    assert lib.gcs_segment_csr_backward(1, 10, 0, 1, 4, 0, None, 1, None) < 0
    assert lib.gcs_segment_csr_backward(1, 10, 3, 1, 4, 0, None, None, None) < 0


def test_drop_ins_import_and_construct():
    import spconv.pytorch as spconv
    import torch_scatter
    from gaussiancity_amd import sparse as SP
    assert spconv.modules.is_spconv_module(spconv.SubMConv3d(4, 4, 3))
    assert not spconv.modules.is_spconv_module(torch.nn.Linear(4, 4))
    assert torch_scatter.segment_csr is SP.segment_csr
    m = spconv.SubMConv3d(128, 32, 5, bias=False, indice_key="stem")
    assert tuple(m.weight.shape) == (32, 5, 5, 5, 128) and m.bias is None
    assert list(m.state_dict()) == ["weight"]
    m = spconv.SubMConv3d(7, 9, kernel_size=3, padding=1, bias=True, indice_key="stage0", algo="native", fp32_accum=True)
    assert tuple(m.weight.shape) == (9, 3, 3, 3, 7) and tuple(m.bias.shape) == (9,)
    assert list(m.state_dict()) == ["weight", "bias"]
    m.load_state_dict({"weight": torch.zeros(9, 3, 3, 3, 7), "bias": torch.ones(9)})
    assert tuple(spconv.SubMConv3d(2, 3, (3, 1, 5)).weight.shape) == (3, 3, 1, 5, 2)
    with pytest.raises(ValueError):
        spconv.SubMConv3d(4, 4, 4)
    with pytest.raises(ValueError):
        spconv.SubMConv3d(4, 4, (3, 2, 3))
    with pytest.raises(ValueError):
        spconv.SubMConv3d(4, 4, 3, stride=2)
    with pytest.raises(ValueError):
        spconv.SubMConv3d(4, 4, 3, groups=2)


def test_sparse_conv_tensor_shares_its_rulebook_dict():
    import spconv.pytorch as spconv
    idx = torch.tensor([[0, 1, 2, 3], [1, 0, 0, 0]], dtype=torch.int32)
    t = spconv.SparseConvTensor(torch.ones(2, 3), idx, [4, 4, 4], 2)
    u = t.replace_feature(torch.zeros(2, 5))
    assert u.indices is t.indices and u.indice_dict is t.indice_dict and u.spatial_shape == [4, 4, 4]
    assert u.batch_size == 2 and tuple(u.features.shape) == (2, 5)
    d = t.dense()
    assert tuple(d.shape) == (2, 3, 4, 4, 4) and float(d[0, :, 1, 2, 3].sum()) == 3 and float(d.sum()) == 6


def test_errors_of_the_python_layer_without_a_gpu():
    import spconv.pytorch as spconv
    import torch_scatter
    idx = torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(TypeError):
        spconv.SubMConv3d(2, 2, 3)(spconv.SparseConvTensor(torch.zeros(3, 2, dtype=torch.float64), idx, [4, 4, 4], 1))
    with pytest.raises(NotImplementedError):
        torch_scatter.segment_csr(torch.zeros(4), torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        torch_scatter.segment_csr(torch.zeros(4), torch.tensor([0, 4]), out=torch.zeros(1))
    with pytest.raises(TypeError):
        torch_scatter.segment_csr(torch.zeros(4, dtype=torch.float64), torch.tensor([0, 4]))
    with pytest.raises(ValueError):
        torch_scatter.segment_csr(torch.zeros(4), torch.tensor([0, 4]), reduce="mul")


def _cloud(seed, n, ext):
    rng = np.random.default_rng(seed)
    coords = np.unique(rng.integers(0, ext, (n, 3)), axis=0)
    batch = rng.integers(0, 2, len(coords))
    idx = R.with_batch(coords, batch)
    # rows must be distinct voxels for the dense comparison: dedupe (b, p)
    _, keep = np.unique(R.pack(idx, (ext,) * 3), return_index=True)
    return idx[np.sort(keep)]


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("dil", [1, 2])
def test_reference_agrees_with_dense_conv3d(k, dil):
    ext = 9
    idx = _cloud(10 * k + dil, 300, ext)
    rng = np.random.default_rng(k * dil)
    cin, cout = 3, 4
    x = rng.normal(size=(len(idx), cin))
    w = rng.normal(size=(cout, k, k, k, cin))
    b = rng.normal(size=cout)
    nbr = R.neighbours(idx, (ext,) * 3, (k,) * 3, (dil,) * 3)
    y, sc = R.conv_forward(x, w, b, nbr)
    want = R.dense_conv_check(x, w, b, idx, (ext,) * 3, 2, (dil,) * 3)
    assert np.abs(y - want).max() <= 1e-12 * max(1.0, sc.max())
    assert (nbr >= 0).sum() > len(idx) * 2                      # the neighbourhoods are not empty
    # the backward formulas are the adjoint of the forward: <dy, f(x)> = <dx, x> (no bias), <dy, f> linear in w
    dy = rng.normal(size=y.shape)
    (dx, _), (dw, _), (db, _) = R.conv_backward(x, w, nbr, dy)
    y0, _ = R.conv_forward(x, w, None, nbr)
    assert abs((dy * y0).sum() - (dx * x).sum()) <= 1e-9 * np.abs(dy * y0).sum()
    assert abs((dy * y0).sum() - (dw * w).sum()) <= 1e-9 * np.abs(dy * y0).sum()
    assert np.allclose(db, dy.sum(0))


def test_reference_duplicate_rule_and_segment_csr():
    idx = np.array([[0, 1, 1, 1], [0, 1, 1, 2], [0, 1, 1, 1], [0, 1, 1, 3]], np.int32)
    nbr = R.neighbours(idx, (4, 4, 4), (3, 3, 3), (1, 1, 1))
    assert nbr[0, 13] == 0 and nbr[2, 13] == 0 and nbr[1, 12] == 0 and nbr[3, 13] == 3 and nbr[3, 12] == 1
    assert np.array_equal(nbr[0], nbr[2]) and not (nbr == 2).any()
    src = np.array([[1.0, 5.0], [3.0, 5.0], [3.0, 2.0], [0.0, 0.0]])
    ip = np.array([0, 3, 3, 4])
    out, _, arg = R.segment_csr(src, ip, "max")
    assert np.array_equal(out, [[3, 5], [0, 0], [0, 0]]) and np.array_equal(arg, [[1, 0], [-1, -1], [3, 3]])
    d = R.segment_csr_backward(np.ones((3, 2)), ip, "max", arg, src.shape)
    assert np.array_equal(d, [[0, 1], [1, 0], [0, 0], [1, 1]])
    out, _, _ = R.segment_csr(src, ip, "mean")
    assert np.allclose(out, [[7 / 3, 4], [0, 0], [0, 0]])
