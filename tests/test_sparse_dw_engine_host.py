"""The weight gradient of the matrix-core engine (include/gcs.h ABI v4), host side (not gpu; no
device is touched): gcs_engine_products and its Python wrappers, the dW counters of sparse.stats(), and the plan and
workspace of every shape that tests/test_sparse_dw_engine_gpu.py runs -- the dW tile and slice count that file was
written for, the same under both engines, and a backward workspace that grows by the dX slices only."""
import pytest

from gaussiancity_amd import _native_s as S
from test_sparse_dw_engine_gpu import SHAPES


def _align(b):
    return (b + 255) // 256 * 256


def test_engine_products_through_the_c_abi():
    L = S.lib()
    assert (S.PRODUCT_FORWARD, S.PRODUCT_DX, S.PRODUCT_DW) == (1, 2, 4)
    assert L.gcs_engine_products(S.ENGINE_VALU) == 0
    assert L.gcs_engine_products(S.ENGINE_MFMA) == 7 == S.PRODUCT_FORWARD | S.PRODUCT_DX | S.PRODUCT_DW
    for unknown in (2, -1):
        assert L.gcs_engine_products(unknown) == -1
        assert L.gcs_last_error() == b"gcs_engine_products: unknown engine (GCS_ENGINE_VALU or GCS_ENGINE_MFMA)"
    assert L.gcs_abi_version() == S.ABI_VERSION == 4


def test_engine_products_wrappers():
    from gaussiancity_amd import sparse as SP
    assert S.engine_products(S.ENGINE_VALU) == 0 and S.engine_products(S.ENGINE_MFMA) == 7
    for unknown in (2, -1):
        with pytest.raises(RuntimeError, match="gcs_engine_products: unknown engine"):
            S.engine_products(unknown)
    assert SP.engine_products("valu") == ()
    assert SP.engine_products("mfma") == ("forward", "dx", "dw")
    with pytest.raises(ValueError, match="valu.*mfma"):
        SP.engine_products("tensor")
    first = SP.get_engine()
    try:
        for name in ("mfma", "valu"):
            SP.set_engine(name)
            assert SP.engine_products() == SP.engine_products(name)
    finally:
        SP.set_engine(first)


def test_stats_count_weight_gradients_per_engine_and_reset():
    from gaussiancity_amd import sparse as SP
    keys = ("conv_dw_calls_valu", "conv_dw_calls_mfma")
    before = SP.stats()
    assert all(k in before for k in keys)
    try:
        SP._STATS["conv_dw_calls_mfma"] += 3
        SP._STATS["conv_dw_calls_valu"] += 2
        after = SP.stats()
        assert after["conv_dw_calls_mfma"] == before["conv_dw_calls_mfma"] + 3
        assert after["conv_dw_calls_valu"] == before["conv_dw_calls_valu"] + 2
        SP.reset_stats()
        assert all(v == 0 for v in SP.stats().values())
    finally:
        SP.reset_stats()


@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_and_workspace_of_the_gpu_files_shapes(name):
    rows, cin, cout, k, tile, slices = SHAPES[name]
    K = k ** 3
    valu = S.subm_engine_plan(S.ENGINE_VALU, rows, cin, cout, K)
    mfma = S.subm_engine_plan(S.ENGINE_MFMA, rows, cin, cout, K)
    assert len(valu) == len(mfma) == 7
    assert (valu[2], valu[3]) == (getattr(S, tile), slices), valu
    assert (mfma[2], mfma[3]) == (valu[2], valu[3]) and mfma[:5] == S.subm_plan(rows, cin, cout, K)
    for dups in (0, 1):
        old = S.lib().gcs_subm_backward_workspace_bytes(rows, cin, cout, K, dups)
        assert S.subm_engine_workspace_bytes(S.ENGINE_VALU, rows, cin, cout, K, dups)[1] == old > 0
        dx_slices = _align(4 * mfma[6] * rows * cin) if mfma[6] > 1 else 0
        assert S.subm_engine_workspace_bytes(S.ENGINE_MFMA, rows, cin, cout, K, dups)[1] == old + dx_slices
