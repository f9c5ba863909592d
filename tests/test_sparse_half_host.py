"""No GPU: the host side of the float16 path of libgcs_hip.so (the `_t` entry points of include/gcs.h, DESIGN.md section
15): the exports and the dtype query, the argument errors that must return before any HIP call, the workspace sizes, the
dtype errors of the Python layer and the new counters.  The kernels are checked by test_sparse_half_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_ref as R


@pytest.fixture(scope="module")
def S():
    from gaussiancity_amd import _native_s
    _native_s.lib()
    return _native_s


TYPED = ["gcs_dtypes", "gcs_subm_workspace_bytes_t", "gcs_subm_forward_t", "gcs_subm_backward_t",
         "gcs_segment_csr_forward_t", "gcs_segment_csr_backward_t"]


def test_exports_and_the_dtype_query(S):
    exported = set(S.EXPORTED_SYMBOLS() if callable(S.EXPORTED_SYMBOLS) else S.EXPORTED_SYMBOLS)
    for name in TYPED:
        assert name in exported, name
        assert name in S._SIGNATURES and hasattr(S.lib(), name), name
    assert S.lib().gcs_dtypes() == 3
    assert S.lib().gcs_abi_version() == 4 == S.ABI_VERSION
    assert S.DTYPES == {"float32": 0, "float16": 1}
    from gaussiancity_amd import sparse as SP
    assert SP.dtypes() == ("float32", "float16")


def _err(S):
    return S.lib().gcs_last_error().decode()


def test_an_unknown_dtype_is_refused_by_every_typed_call(S):
    L = S.lib()
    f, b = C.c_size_t(0), C.c_size_t(0)
    for dtype in (2, -1, 7):
        assert L.gcs_subm_workspace_bytes_t(dtype, 100, 4, 4, 27, 0, C.byref(f), C.byref(b)) == -1
        assert "unknown dtype" in _err(S) and "gcs_subm_workspace_bytes_t" in _err(S)
        assert L.gcs_subm_forward_t(dtype, 0x1000, 100, 27, 0x2000, 4, 0x3000, None, 4, 0x4000, None, 0, None) == -1
        assert "gcs_subm_forward_t: unknown dtype" in _err(S)
        assert L.gcs_subm_backward_t(dtype, 0x1000, 100, 27, 0, 0x2000, 4, 0x3000, 4, 0x4000, 0x5000, None, None, 0x6000,
                                     1 << 30, None) == -1
        assert "gcs_subm_backward_t: unknown dtype" in _err(S)
        assert L.gcs_segment_csr_forward_t(dtype, 0x1000, 4, 4, 0x2000, 1, 0, 0x3000, None, None) == -1
        assert "gcs_segment_csr_forward_t: unknown dtype" in _err(S)
        assert L.gcs_segment_csr_backward_t(dtype, 0x1000, 4, 4, 0x2000, 1, 0, None, 0x3000, None) == -1
        assert "gcs_segment_csr_backward_t: unknown dtype" in _err(S)


def test_an_odd_binary16_pointer_is_refused_before_anything_is_queued(S):
    """The pointers are made-up addresses: a call that got past the argument checks would hand them to a kernel."""
    L = S.lib()
    F16 = S.DTYPE_F16
    good = dict(x=0x2000, w=0x3000, b=0x3800, y=0x4000)
    for odd in good:
        a = dict(good)
        a[odd] += 1
        assert L.gcs_subm_forward_t(F16, 0x1000, 100, 27, a["x"], 4, a["w"], a["b"], 4, a["y"], None, 0, None) == -1, odd
        assert "2-byte aligned" in _err(S)
    good = dict(x=0x2000, w=0x3000, dy=0x4000, dx=0x5000, dw=0x6000, db=0x7000)
    for odd in good:
        a = dict(good)
        a[odd] += 1
        assert L.gcs_subm_backward_t(F16, 0x1000, 100, 27, 0, a["x"], 4, a["w"], 4, a["dy"], a["dx"], a["dw"], a["db"],
                                     0x8000, 1 << 30, None) == -1, odd
        assert "2-byte aligned" in _err(S)
    assert L.gcs_segment_csr_forward_t(F16, 0x1001, 4, 4, 0x2000, 1, 0, 0x3000, None, None) == -1
    assert "2-byte aligned" in _err(S)
    assert L.gcs_segment_csr_forward_t(F16, 0x1000, 4, 4, 0x2000, 1, 0, 0x3001, None, None) == -1
    assert L.gcs_segment_csr_backward_t(F16, 0x1001, 4, 4, 0x2000, 1, 0, None, 0x3000, None) == -1
    assert L.gcs_segment_csr_backward_t(F16, 0x1000, 4, 4, 0x2000, 1, 0, None, 0x3001, None) == -1
    assert "2-byte aligned" in _err(S)


def test_a_missing_workspace_is_refused_where_the_plan_needs_one(S):
    L = S.lib()
    n, c, K = 73, 512, 27                                       # PTv3's stage 4: forward and dX in tap slices
    plan = S.subm_engine_plan(S.ENGINE_MFMA, n, c, c, K)
    assert plan[5] > 1 and plan[6] > 1
    fwd, bwd = S.subm_workspace_bytes_t(S.DTYPE_F16, n, c, c, K, 0)
    assert fwd > 0 and bwd > 0
    args = (S.DTYPE_F16, 0x1000, n, K, 0x2000, c, 0x3000, None, c, 0x4000)
    assert L.gcs_subm_forward_t(*args, None, 0, None) == -1 and "workspace" in _err(S)
    assert L.gcs_subm_forward_t(*args, 0x10000, fwd - 1, None) == -1 and "workspace" in _err(S)
    bargs = (S.DTYPE_F16, 0x1000, n, K, 0, 0x2000, c, 0x3000, c, 0x4000, 0x5000, None, None)
    assert L.gcs_subm_backward_t(*bargs, None, 0, None) == -1 and "workspace" in _err(S)
    assert L.gcs_subm_backward_t(*bargs, 0x10000, bwd - 1, None) == -1 and "workspace" in _err(S)
    # the workspace holds fp32 partials: a base that is not 4-byte aligned is refused too
    assert L.gcs_subm_forward_t(*args, 0x10002, fwd, None) == -1 and "4-byte aligned" in _err(S)
    assert L.gcs_subm_backward_t(*bargs, 0x10002, bwd, None) == -1 and "4-byte aligned" in _err(S)
    # the backward always needs one (the dB partials), sliced or not
    assert S.subm_engine_plan(S.ENGINE_MFMA, 16384, 32, 32, K)[5:] == (1, 1)
    assert L.gcs_subm_backward_t(S.DTYPE_F16, 0x1000, 16384, K, 0, 0x2000, 32, 0x3000, 32, 0x4000, 0x5000, None, None, None,
                                 0, None) == -1 and "workspace" in _err(S)
    # float32 through the typed call: the default backward's rule
    assert L.gcs_subm_backward_t(S.DTYPE_F32, 0x1000, n, K, 0, 0x2000, c, 0x3000, c, 0x4000, 0x5000, None, None, None, 0,
                                 None) == -1 and "workspace" in _err(S)


def _grid():
    shell = R.pool_stages(R.shell_cloud(16384, 2024), 4)
    shapes = [(len(shell[stage]), cin, cout, k ** 3) for cin, cout, k, stage in R.PTV3_SHAPES]
    shapes += [(n, cin, cout, K) for n in (0, 1, 73, 300, 2469, 5500, 32805, 262144)
               for cin, cout in ((1, 1), (6, 5), (37, 21), (64, 70), (136, 200), (20, 24)) for K in (1, 15, 27)]
    return shapes


def test_workspace_sizes(S):
    L = S.lib()
    for n, cin, cout, K in _grid():
        for dups in (0, 1):
            f32 = S.subm_workspace_bytes_t(S.DTYPE_F32, n, cin, cout, K, dups)
            assert f32 == (0, L.gcs_subm_backward_workspace_bytes(n, cin, cout, K, dups)), (n, cin, cout, K, dups)
            f16 = S.subm_workspace_bytes_t(S.DTYPE_F16, n, cin, cout, K, dups)
            eng = S.subm_engine_workspace_bytes(S.ENGINE_MFMA, n, cin, cout, K, dups)
            assert f16[0] <= eng[0] and f16[1] <= eng[1], (n, cin, cout, K, dups, f16, eng)
            plan = S.subm_engine_plan(S.ENGINE_MFMA, max(n, 0), cin, cout, K)
            assert (f16[0] > 0) == (plan[5] > 1 and n > 0)
            if dups and n * cout >= 256:                        # below that the 256-byte granule hides it
                assert f16[1] < eng[1], "the binary16 fold is half the float one"
    f, b = C.c_size_t(0), C.c_size_t(0)
    assert L.gcs_subm_workspace_bytes_t(S.DTYPE_F16, -1, 4, 4, 27, 0, C.byref(f), C.byref(b)) == -1
    assert L.gcs_subm_workspace_bytes_t(S.DTYPE_F16, 10, 4, 4, 27, 0, None, C.byref(b)) == -1


def _tensor(dtype, rows=3, ch=2):
    idx = torch.zeros(rows, 4, dtype=torch.int32)
    import spconv.pytorch as spconv
    return spconv.SparseConvTensor(torch.zeros(rows, ch, dtype=dtype), idx, [4, 4, 4], 1)


def test_dtype_errors_of_the_python_layer_without_a_gpu():
    import spconv.pytorch as spconv
    import torch_scatter
    with pytest.raises(RuntimeError, match="GPU"):              # the dtype is accepted; the device is not
        spconv.SubMConv3d(2, 2, 3).half()(_tensor(torch.float16))
    with pytest.raises(RuntimeError, match="GPU"):
        torch_scatter.segment_csr(torch.zeros(4, dtype=torch.float16), torch.tensor([0, 4]))
    for bad in (torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="float32.*float16|float16.*float32"):
            spconv.SubMConv3d(2, 2, 3)(_tensor(bad))
        with pytest.raises(TypeError, match="float32.*float16|float16.*float32"):
            spconv.SubMConv3d(2, 2, 3).to(bad)(_tensor(bad))
        with pytest.raises(TypeError, match="float32.*float16|float16.*float32"):
            torch_scatter.segment_csr(torch.zeros(4, dtype=bad), torch.tensor([0, 4]))
    assert not torch.is_autocast_enabled()
    with pytest.raises(TypeError, match="one dtype"):           # mixed, no autocast
        spconv.SubMConv3d(2, 2, 3)(_tensor(torch.float16))
    with pytest.raises(TypeError, match="one dtype"):
        spconv.SubMConv3d(2, 2, 3).half()(_tensor(torch.float32))
    conv = spconv.SubMConv3d(2, 2, 3).half()
    conv.bias.data = conv.bias.data.float()
    with pytest.raises(TypeError, match="one dtype"):
        conv(_tensor(torch.float16))


def test_the_half_counters_exist_and_reset():
    from gaussiancity_amd import sparse as SP
    st = SP.stats()
    assert "conv_forward_calls_half" in st and "conv_dw_calls_half" in st
    SP._STATS["conv_forward_calls_half"] += 3
    SP._STATS["conv_dw_calls_half"] += 2
    assert SP.stats()["conv_forward_calls_half"] >= 3
    SP.reset_stats()
    assert set(SP.stats().values()) == {0}


def test_the_bar_holds_for_an_fp32_accumulate_round_once_emulation():
    """The unit of test_sparse_half_gpu.py, 2^-11 * A + 2^-24, checked against the contract on the CPU: binary16 operands,
    a float32 sum over (tap, channel), the bias added last, one rounding.  Shows the bar is the contract's, not the GPU's."""
    n, cin, cout = 300, 6, 5
    coords = R.shell_cloud(n, n + cin, extent=48)
    idx = R.with_batch(coords, np.random.default_rng(n).integers(0, 2, n))
    rng = np.random.default_rng(cin)
    x = rng.normal(size=(n, cin)).astype(np.float16)
    w = (rng.normal(size=(cout, 3, 3, 3, cin)) / np.sqrt(27 * cin)).astype(np.float16)
    b = rng.normal(size=cout).astype(np.float16)
    nbr = R.neighbours(idx, [48] * 3, (3, 3, 3), (1, 1, 1))
    ry, sy = R.conv_forward(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), nbr)
    acc = np.zeros((n, cout), np.float32)
    W = w.reshape(cout, 27, cin).astype(np.float32)
    for k in range(27):
        m = nbr[:, k] >= 0
        for c in range(cin):
            acc[m] += x[nbr[m, k], c].astype(np.float32)[:, None] * W[None, :, k, c]
    got = (acc + b.astype(np.float32)).astype(np.float16).astype(np.float64)
    ratio = np.abs(got - ry) / (2.0 ** -11 * sy + 2.0 ** -24)
    assert ratio.max() <= 2.0, ratio.max()
